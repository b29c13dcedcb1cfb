"""Learning-rate schedules with warm-up: the host side.

The DreamBooth script builds diffusers' `get_scheduler(args.lr_scheduler, num_warmup_steps=args.lr_warmup_steps *
num_processes, num_training_steps=args.max_train_steps * num_processes, num_cycles=args.lr_num_cycles,
power=args.lr_power)` (DB:586-612, 1614-1621) and steps it once per optimizer step (DB:1962-1963).  LrSchedule is the
lambda of that scheduler: `lr_k = base_lr * multiplier(k)`, k = the optimizer steps already applied, so the first step
runs at multiplier(0).  A step the loss scaler skips does not advance k (accelerate's scheduler wrapper skips when the
optimizer step was skipped); a Prodigy step that ends early at a zero denominator does -- the schedule counts the
optimizer steps the scaler let through, not Prodigy's own k, or a warm-up from 0 would never leave 0.

World size cancels.  The script multiplies the warm-up and the total by num_processes, and accelerate's wrapper steps
the scheduler num_processes times per optimizer step: the lambdas then see (k W, w W, T W), and every quotient they
form -- k W / (w W), (T W - k W) / (T W - w W), (k W - w W) / (T W - w W) -- is the same rational number as without W,
correctly rounded to the same double.  So every rank evaluates multiplier(k) with the unscaled counts.

The expressions are those of diffusers' optimization.py in double, term for term (transformers.optimization carries
the same six lambdas and is what the tests compare against; parity with diffusers itself is unpinned: DESIGN.md
section 7 #13).  csrc/optim.hip's pso_lr_schedule evaluates the same expressions on the device, where the applied-step
count lives when an amp.DeviceLossScaler trains (kernels.lr_schedule); the lr a kernel receives is
float32(base_lr * multiplier(k)) on the host and on the device alike.
"""
import math
import struct

from ._lib import LR_KINDS

LR_END = 1e-7  # get_scheduler does not pass lr_end: the polynomial kind always decays to diffusers' default
_DECAYING = ("linear", "cosine", "cosine_with_restarts", "polynomial")


class LrSchedule:
    def __init__(self, kind, base_lr, num_warmup_steps=0, num_training_steps=None, num_cycles=1, power=1.0):
        self._set(kind, base_lr, num_warmup_steps, num_training_steps, num_cycles, power)

    def _set(self, kind, base_lr, num_warmup_steps, num_training_steps, num_cycles, power):
        kind = str(kind)
        if kind not in LR_KINDS:  # diffusers' piecewise_constant included: it needs step rules the script never passes
            raise ValueError(f"lr_scheduler must be one of {sorted(LR_KINDS)}, got {kind!r}")
        base_lr, warmup = float(base_lr), int(num_warmup_steps)
        if not base_lr > 0.0:
            raise ValueError(f"lr_scheduler={kind!r}: the base learning rate must be positive, got {base_lr!r}")
        if warmup < 0:
            raise ValueError(f"lr_warmup_steps must be >= 0, got {num_warmup_steps!r}")
        if kind in _DECAYING and num_training_steps is None:
            raise ValueError(f"lr_scheduler={kind!r} decays towards the end of training: it needs max_train_steps")
        total = 0 if num_training_steps is None else int(num_training_steps)
        if kind == "polynomial":
            if not base_lr > LR_END:  # diffusers' own check
                raise ValueError(f"lr_end ({LR_END}) must be smaller than initial lr ({base_lr})")
            if total <= warmup:  # diffusers divides by zero at the first decay step
                raise ValueError(f"lr_scheduler='polynomial' needs max_train_steps ({total}) > lr_warmup_steps "
                                 f"({warmup})")
        self.kind, self.base_lr, self.num_warmup_steps = kind, base_lr, warmup
        self.num_training_steps = None if num_training_steps is None else total
        self.num_cycles, self.power = int(num_cycles), float(power)

    @property
    def kind_code(self):
        return LR_KINDS[self.kind]

    def multiplier(self, k):
        """lambda(k) in double, the expressions of diffusers' optimization.py."""
        k, w, T = int(k), self.num_warmup_steps, self.num_training_steps
        if self.kind == "constant":  # ignores the warm-up, as diffusers does
            return 1.0
        if k < w:
            return float(k) / float(max(1, w))
        if self.kind == "constant_with_warmup":
            return 1.0
        if self.kind == "linear":
            return max(0.0, float(T - k) / float(max(1, T - w)))
        if self.kind == "polynomial":
            if k > T:
                return LR_END / self.base_lr
            pct_remaining = 1 - (k - w) / (T - w)
            return ((self.base_lr - LR_END) * pct_remaining ** self.power + LR_END) / self.base_lr
        progress = float(k - w) / float(max(1, T - w))
        if self.kind == "cosine":  # get_scheduler does not pass num_cycles to this kind: 0.5; rises again past T
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
        if progress >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(self.num_cycles) * progress) % 1.0))))

    def lr(self, k):
        """base_lr * lambda(k) in double; a kernel receives it rounded to float32 once (lr32)."""
        return self.base_lr * self.multiplier(k)

    def lr32(self, k):
        """The float32 value the optimizer kernels run step k + 1 at, as a Python float."""
        return struct.unpack("f", struct.pack("f", self.lr(k)))[0]

    def state_dict(self):
        return {"kind": self.kind, "base_lr": self.base_lr, "num_warmup_steps": self.num_warmup_steps,
                "num_training_steps": self.num_training_steps, "num_cycles": self.num_cycles, "power": self.power}

    def load_state_dict(self, sd):
        self._set(sd["kind"], sd["base_lr"], sd["num_warmup_steps"], sd["num_training_steps"], sd["num_cycles"],
                  sd["power"])


def make_lr_schedule(lr_scheduler, base_lr, lr_warmup_steps=0, max_train_steps=None, lr_num_cycles=1, lr_power=1.0):
    """The schedule both trainers build from their lr_* arguments: None for "constant" (the trainer then runs the
    fixed-rate code as it always has: same entries, same launches), else an LrSchedule.  An unknown name raises
    ValueError naming lr_scheduler, a decaying kind without max_train_steps one naming max_train_steps."""
    if str(lr_scheduler) == "constant":
        return None
    return LrSchedule(lr_scheduler, base_lr, lr_warmup_steps, max_train_steps, lr_num_cycles, lr_power)
