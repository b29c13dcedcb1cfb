"""Dynamic loss scaling for fp16 training (the f16 library, PSO_LIB=f16).

The reference recipes train under accelerate's `mixed_precision="fp16"`: the loss is multiplied by a scale before
backward so that small activation gradients survive fp16's narrow exponent range, the gradient is divided by it again
before clipping, and a step whose gradient holds an inf / NaN is skipped and the scale backed off (torch's GradScaler,
T:303-319, 344-350).  LossScaler is that state machine on the host, with GradScaler's semantics and defaults; the
trainer (trainer.lora_optimizer_step) supplies `found_inf` from the all-reduced gradient norm, its one sync per
optimizer step.  The scale stays a power of two, so multiplying and dividing by it is exact.

DeviceLossScaler is the same state machine with its state in device memory, as GradScaler keeps it: the kernels of
csrc/optim.hip (include/pso_amd.h, PSO_AMP_*) unscale, detect the inf, skip or apply the optimizer step and update the
scale, so an optimizer step reads nothing back and a captured epoch serves every scale.
"""
import torch

from . import _lib


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


class DeviceLossScaler:
    """LossScaler with the state block of include/pso_amd.h (PSO_AMP_WORDS four-byte words: scale, 1 / scale,
    found_inf, growth tracker, applied and skipped step counts, the last norm and clip coefficient, the step's
    bias-correction constants) on `device`.  Reading `.scale`, `.skipped`, `.growth_tracker`, `.step` or `state_dict()`
    copies the block to the host -- a sync, by request only; the trainers never do it inside a step."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, device=None):
        if not (init_scale > 0.0 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and growth_interval >= 1):
            raise ValueError("DeviceLossScaler: need init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1, "
                             "growth_interval >= 1")
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        host = torch.zeros(_lib.AMP_WORDS, dtype=torch.int32)
        self._put_scale(host, float(init_scale))
        self.state = host.to("cuda" if device is None else device)  # int32 words; float words through .view(float32)

    @staticmethod
    def _put_scale(words, scale):
        f = words.view(torch.float32)
        f[_lib.AMP_SCALE] = scale
        f[_lib.AMP_INV_SCALE] = 1.0 / f[_lib.AMP_SCALE]  # fp32 reciprocal of the fp32 scale, as the update kernel's

    @property
    def scale_word(self):
        """The fp32 scale as a one-element device tensor: `grad_out` of the loss backward kernels."""
        return self.state.view(torch.float32)[_lib.AMP_SCALE:_lib.AMP_SCALE + 1]

    def _host(self):
        return self.state.cpu()

    def _write(self, host):
        self.state.copy_(host)

    @property
    def scale(self):
        return float(self._host().view(torch.float32)[_lib.AMP_SCALE])

    @scale.setter
    def scale(self, value):
        host = self._host()
        self._put_scale(host, float(value))
        self._write(host)

    @property
    def growth_tracker(self):
        return int(self._host()[_lib.AMP_GROWTH_TRACKER])

    @property
    def skipped(self):
        return int(self._host()[_lib.AMP_SKIPPED])

    @property
    def step(self):
        """Applied optimizer steps (AdamW's step count; a skipped step does not count)."""
        return int(self._host()[_lib.AMP_STEP])

    @step.setter
    def step(self, value):
        host = self._host()
        host[_lib.AMP_STEP] = int(value)
        self._write(host)

    def state_dict(self):
        host = self._host()
        return {"scale": float(host.view(torch.float32)[_lib.AMP_SCALE]), "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval,
                "growth_tracker": int(host[_lib.AMP_GROWTH_TRACKER]), "skipped": int(host[_lib.AMP_SKIPPED]),
                "step": int(host[_lib.AMP_STEP])}

    def load_state_dict(self, sd):
        """Accepts a LossScaler's state_dict as well (no "skipped" / "step": those counts are kept)."""
        self.growth_factor = float(sd["growth_factor"])
        self.backoff_factor = float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        host = self._host()
        self._put_scale(host, float(sd["scale"]))
        host[_lib.AMP_GROWTH_TRACKER] = int(sd["growth_tracker"])
        for key, word in (("skipped", _lib.AMP_SKIPPED), ("step", _lib.AMP_STEP)):
            if key in sd:
                host[word] = int(sd[key])
        self._write(host)


def make_scaler(loss_scale):
    """None | float | LossScaler | DeviceLossScaler -> a scaler or None (a float is the initial scale of a host
    LossScaler)."""
    if loss_scale is None or isinstance(loss_scale, (LossScaler, DeviceLossScaler)):
        return loss_scale
    return LossScaler(init_scale=float(loss_scale))
