"""numpy restatement of the Prodigy step (prodigyopt 1.0's Prodigy.step, one parameter group) as include/pso_amd.h
documents pso_prodigy_step.  Parity with the package is unpinned: prodigyopt is not installed here.

Per-element state (m, v, s, p0, p) is float32 and every elementwise operation rounds to float32 in the order of the
header; the two sums and all scalar algebra are float64, and a scalar enters the elementwise arithmetic rounded to
float32 once.  Hyper-parameters are the float32 values the C-ABI receives (tests/test_gpu_optim.py's LR, B1, ...).
"""
import math

import numpy as np

f32 = np.float32


class ProdigyRef:
    def __init__(self, p, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                 use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
        self.p = np.array(p, dtype=f32).copy()
        self.p0 = self.p.copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.s = np.zeros_like(self.p)
        self.lr, self.b1, self.b2 = f32(lr), f32(betas[0]), f32(betas[1])
        self.b3 = f32(math.sqrt(float(betas[1])) if beta3 is None else beta3)
        self.eps, self.wd = f32(eps), f32(weight_decay)
        self.d_coef, self.growth_rate = f32(d_coef), f32(growth_rate)
        self.decouple, self.bias, self.safeguard = bool(decouple), bool(use_bias_correction), bool(safeguard_warmup)
        self.d = self.d0 = self.d_max = float(d0)
        self.d_numerator = 0.0
        self.d_denom = self.d_hat = self.dlr = 0.0
        self.k = 0
        self.updated = 0
        # |num| against the sum of the absolute values of its terms, of the last step (the cancellation in d_hat)
        self.num_abs_terms = 0.0

    def scalars(self):
        return {"d": self.d, "d0": self.d0, "d_max": self.d_max, "d_numerator": self.d_numerator,
                "d_denom": self.d_denom, "d_hat": self.d_hat, "dlr": self.dlr, "k": self.k, "updated": self.updated}

    def step(self, grad, gmul=1.0):
        """grad float32, gmul = the float32 factor the kernel puts on the gradient read (grad_scale * clip)."""
        b1, b2, b3 = float(self.b1), float(self.b2), float(self.b3)
        d, d0 = self.d, self.d0
        bc = 1.0
        if self.bias:
            bc = math.sqrt(1.0 - b2 ** (self.k + 1)) / (1.0 - b1 ** (self.k + 1))
        dlr = d * float(self.lr) * bc
        g = np.asarray(grad, dtype=f32) * f32(gmul)
        if not self.decouple and self.wd != 0:
            g = g + self.wd * self.p
        # pass 1, with the d the step started from
        terms = g.astype(np.float64) * (self.p0.astype(np.float64) - self.p.astype(np.float64))
        dot = float(terms.sum())
        cm = f32(d * (1.0 - b1))
        cv = f32(d * d * (1.0 - b2))
        cs = f32((d / d0) * (d if self.safeguard else dlr))
        self.m = self.b1 * self.m + cm * g
        self.v = self.b2 * self.v + (cv * g) * g
        self.s = self.b3 * self.s + cs * g
        den = float(np.abs(self.s).astype(np.float64).sum())
        w = (d / d0) * dlr
        num = b3 * self.d_numerator + w * dot
        self.num_abs_terms = abs(b3 * self.d_numerator) + abs(w) * float(np.abs(terms).sum())
        self.num_last = num
        self.dlr, self.d_denom = dlr, den
        if den == 0.0:
            self.updated = 0
            return
        d_hat = float(self.d_coef) * num / den
        if d == d0:
            d = max(d, d_hat)
        self.d_max = max(self.d_max, d_hat)
        d = min(self.d_max, d * float(self.growth_rate))
        self.d, self.d_numerator, self.d_hat = d, num, d_hat
        self.k += 1
        self.updated = 1
        # pass 2, with the new d and the dlr from above
        if self.decouple and self.wd != 0:
            self.p = self.p - f32(float(self.wd) * dlr) * self.p
        self.p = self.p - (f32(dlr) * self.m) / (np.sqrt(self.v) + f32(d * float(self.eps)))
