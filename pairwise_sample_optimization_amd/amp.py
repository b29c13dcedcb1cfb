"""Dynamic loss scaling for fp16 training (the f16 library, PSO_LIB=f16).

The reference recipes train under accelerate's `mixed_precision="fp16"`: the loss is multiplied by a scale before
backward so that small activation gradients survive fp16's narrow exponent range, the gradient is divided by it again
before clipping, and a step whose gradient holds an inf / NaN is skipped and the scale backed off (torch's GradScaler,
T:303-319, 344-350).  LossScaler is that state machine on the host, with GradScaler's semantics and defaults; the
trainer (trainer.lora_optimizer_step) supplies `found_inf` from the all-reduced gradient norm, its one sync per
optimizer step.  The scale stays a power of two, so multiplying and dividing by it is exact.
"""


class LossScaler:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not (init_scale > 0.0 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and growth_interval >= 1):
            raise ValueError("LossScaler: need init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1, "
                             "growth_interval >= 1")
        self.scale = float(init_scale)
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.growth_tracker = 0  # clean steps since the last change of the scale
        self.skipped = 0         # optimizer steps dropped for a non-finite gradient

    def update(self, found_inf):
        """After one optimizer step attempt: back off on a non-finite gradient (the step was skipped), otherwise count
        towards growth and grow after `growth_interval` clean steps in a row.  Returns the new scale."""
        if found_inf:
            self.scale *= self.backoff_factor
            self.growth_tracker = 0
            self.skipped += 1
        else:
            self.growth_tracker += 1
            if self.growth_tracker == self.growth_interval:
                self.scale *= self.growth_factor
                self.growth_tracker = 0
        return self.scale

    def state_dict(self):
        return {"scale": self.scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "growth_tracker": self.growth_tracker}

    def load_state_dict(self, sd):
        self.scale = float(sd["scale"])
        self.growth_factor = float(sd["growth_factor"])
        self.backoff_factor = float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.growth_tracker = int(sd["growth_tracker"])


def make_scaler(loss_scale):
    """None | float | LossScaler -> LossScaler or None (a float is the initial scale)."""
    if loss_scale is None or isinstance(loss_scale, LossScaler):
        return loss_scale
    return LossScaler(init_scale=float(loss_scale))
