"""numpy restatement of the EMA of the trained weights (pairwise_sample_optimization_amd/ema.py, csrc/ema.hip):
diffusers' EMAModel.get_decay in Python double, and its element update
s_param.sub_(one_minus_decay * (s_param - param)) as three separately rounded float32 operations, one per line."""
import numpy as np


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False,
              inv_gamma=1.0, power=2 / 3):
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur = (1 + step) / (10 + step)
    cur = min(cur, decay)
    cur = max(cur, min_decay)
    return cur


def one_minus_decay32(decay):
    """What the kernel receives: float32(1 - decay), the subtraction in double."""
    return np.float32(1.0 - decay)


def ema_update(shadow, param, one_minus_decay):
    """shadow, param: float32 arrays; one_minus_decay: a float32.  Returns the new shadow (float32)."""
    s = np.asarray(shadow, dtype=np.float32)
    p = np.asarray(param, dtype=np.float32)
    omd = np.float32(one_minus_decay)
    t = (s - p).astype(np.float32)
    u = (omd * t).astype(np.float32)
    out = (s - u).astype(np.float32)
    assert t.dtype == u.dtype == out.dtype == np.float32
    return out
