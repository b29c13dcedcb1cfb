"""Exponential moving average of the trained weights: diffusers' `EMAModel` (the `--use_ema` of its training scripts)
over the ONE flat fp32 master that `trainer.trainable(unet)` returns -- LoRA, the narrow ranks, DoRA with its
magnitudes and the full-UNet mode alike.  diffusers is not installed here: parity with it is unpinned, and the
arithmetic is restated in include/pso_amd.h (pso_ema_step) and tests/ema_ref.py.

  step()     optimization_step += 1; decay = get_decay(optimization_step), all in Python double; one pso_ema_step launch
             with float32(1 - decay): shadow -= (1 - decay) * (shadow - master).  Nothing is read back, and there is
             no device-side scalar: the EMA counts calls of the trainer's optimizer_step, which the host always knows
             (also under amp.DeviceLossScaler, where the applied-step count lives on the device).
  swap()     master <-> shadow in one pass (pso_ema_swap) and the UNet's refresh(), which rebuilds the working copies,
             the transposes and the DoRA norms and bumps the adapter version, so fuse_lora() re-merges.  The exchange
             moves contents, never pointers: the kernels' descriptor tables hold the master's address.  No third
             buffer exists -- in the full-UNet mode the master is 10 GB.
  store() / copy_to() / restore() and average_parameters() are diffusers' names on top of swap(): while the shadow is
  swapped in, the live weights wait in the shadow's buffer, and the owning trainer's micro_step / optimizer_step raise
  (training on the averaged weights would silently corrupt the run).  Swapping back is exact: a swap moves bits.
"""
import contextlib

import numpy as np
import torch

from . import kernels as K

EMA_KEYS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")


def _trainable(unet):
    from .trainer import trainable
    return trainable(unet)


class EMAModel:
    def __init__(self, unet, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
                 power=2 / 3):
        """decay: the cap of the decay; min_decay: its floor; update_after_step: the shadow starts to average after
        that many steps (it follows the master until then); use_ema_warmup / inv_gamma / power: diffusers' warm-up form
        1 - (1 + step / inv_gamma) ** -power instead of (1 + step) / (10 + step)."""
        self._check(decay, min_decay, update_after_step, inv_gamma, power)
        self.unet = unet
        self.decay, self.min_decay = float(decay), float(min_decay)
        self.update_after_step = int(update_after_step)
        self.use_ema_warmup = bool(use_ema_warmup)
        self.inv_gamma, self.power = float(inv_gamma), float(power)
        self.shadow = _trainable(unet)[0].detach().clone()
        self.optimization_step = 0
        self.cur_decay_value = None
        self.swapped = False  # True while the shadow's values sit in the master (and the live weights in self.shadow)

    @staticmethod
    def _check(decay, min_decay, update_after_step, inv_gamma, power):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMAModel: decay must lie in [0, 1], got {decay!r}")
        if not 0.0 <= min_decay <= 1.0:
            raise ValueError(f"EMAModel: min_decay must lie in [0, 1], got {min_decay!r}")
        if not update_after_step >= 0:
            raise ValueError(f"EMAModel: update_after_step must not be negative, got {update_after_step!r}")
        if not inv_gamma > 0.0:
            raise ValueError(f"EMAModel: inv_gamma must be positive, got {inv_gamma!r}")
        if not power >= 0.0:
            raise ValueError(f"EMAModel: power must not be negative, got {power!r}")

    def get_decay(self, optimization_step):
        """The decay of the `optimization_step`-th step (counting from 1), in Python double."""
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur = 1.0 - (1.0 + step / self.inv_gamma) ** -self.power
        else:
            cur = (1.0 + step) / (10.0 + step)
        cur = min(cur, self.decay)
        return max(cur, self.min_decay)

    def step(self):
        """One EMA update towards the current master: one launch, nothing read back."""
        if self.swapped:
            raise RuntimeError("EMAModel.step() while the shadow is swapped in: restore() first")
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        K.ema_step(self.shadow, _trainable(self.unet)[0], float(np.float32(1.0 - decay)))

    # ------------------------------------------------------------------------------------------------------------
    # evaluating / shipping the averaged weights
    # ------------------------------------------------------------------------------------------------------------
    def swap(self):
        """master <-> shadow (contents, one pass) followed by the UNet's refresh()."""
        master, _, refresh = _trainable(self.unet)
        K.ema_swap(master, self.shadow)
        self.swapped = not self.swapped
        refresh()

    def store(self):
        """diffusers' store(): keep the live weights for restore().  They are kept by copy_to()'s exchange itself (in
        the shadow's buffer), so this only checks that no averaged weights are swapped in already."""
        if self.swapped:
            raise RuntimeError("EMAModel.store() while the shadow is already swapped in")

    def copy_to(self):
        """diffusers' copy_to(): the UNet computes with the averaged weights from here on; the live ones wait in the
        shadow's buffer until restore()."""
        if self.swapped:
            raise RuntimeError("EMAModel.copy_to(): the shadow is already swapped in (restore() first)")
        self.swap()

    def restore(self):
        """diffusers' restore(): the live weights back, bit for bit."""
        if not self.swapped:
            raise RuntimeError("EMAModel.restore() without a copy_to(): the live weights are in place")
        self.swap()

    @contextlib.contextmanager
    def average_parameters(self):
        """with ema.average_parameters(): the UNet's forwards (fuse_lora() included) read the averaged weights."""
        self.store()
        self.copy_to()
        try:
            yield self
        finally:
            self.restore()

    # ------------------------------------------------------------------------------------------------------------
    # state
    # ------------------------------------------------------------------------------------------------------------
    def scalars(self):
        return {k: getattr(self, k) for k in EMA_KEYS}

    def load_scalars(self, sd):
        self._check(sd["decay"], sd["min_decay"], sd["update_after_step"], sd["inv_gamma"], sd["power"])
        self.decay, self.min_decay = float(sd["decay"]), float(sd["min_decay"])
        self.optimization_step = int(sd["optimization_step"])
        self.update_after_step = int(sd["update_after_step"])
        self.use_ema_warmup = bool(sd["use_ema_warmup"])
        self.inv_gamma, self.power = float(sd["inv_gamma"]), float(sd["power"])
        self.cur_decay_value = self.get_decay(self.optimization_step) if self.optimization_step else None

    def state_dict(self):
        """diffusers' keys; shadow_params holds the one flat shadow."""
        if self.swapped:
            raise RuntimeError("EMAModel.state_dict() while the shadow is swapped in: restore() first")
        return dict(self.scalars(), shadow_params=[self.shadow.detach().clone()])

    def load_state_dict(self, sd):
        if self.swapped:
            raise RuntimeError("EMAModel.load_state_dict() while the shadow is swapped in: restore() first")
        shadow = sd["shadow_params"]
        if len(shadow) != 1 or shadow[0].numel() != self.shadow.numel():
            raise ValueError("EMAModel.load_state_dict: shadow_params must hold one flat tensor of "
                             f"{self.shadow.numel()} elements")
        self.load_scalars(sd)
        self.shadow.copy_(shadow[0].reshape(self.shadow.shape))

    def state_dict_peft(self):
        """The shadow under LoraState.state_dict_peft()'s names (lora_A / lora_B and, DoRA, lora_magnitude_vector): the
        averaged adapter as a LoRA file of its own.  LoRA training only."""
        st = self._lora("state_dict_peft")
        if self.swapped:
            raise RuntimeError("EMAModel.state_dict_peft() while the shadow is swapped in: restore() first")
        from .unet import MAGNITUDE_KEY
        out = {}
        for name in st.adapter_names():
            A, B = st.adapter_views(self.shadow, name)
            out[f"{name}.lora_A.weight"] = A.detach().clone()
            out[f"{name}.lora_B.weight"] = B.detach().clone()
            if st.dora:
                out[f"{name}.{MAGNITUDE_KEY}.weight"] = st.magnitude_view(self.shadow, name).detach().clone()
        return out

    def load_peft(self, sd):
        """Copy a peft-named state dict (state_dict_peft()'s keys) into the shadow."""
        st = self._lora("load_peft")
        if self.swapped:
            raise RuntimeError("EMAModel.load_peft() while the shadow is swapped in: restore() first")
        from .unet import MAGNITUDE_KEY
        for name in st.adapter_names():
            A, B = st.adapter_views(self.shadow, name)
            A.copy_(sd[f"{name}.lora_A.weight"])
            B.copy_(sd[f"{name}.lora_B.weight"])
            if st.dora:
                k = f"{name}.{MAGNITUDE_KEY}"
                st.magnitude_view(self.shadow, name).copy_(sd.get(k + ".weight", sd.get(k)).reshape(-1))

    def _lora(self, what):
        if getattr(self.unet, "full", None) is not None or getattr(self.unet, "lora", None) is None:
            raise ValueError(f"EMAModel.{what}: the shadow has LoRA names only when the UNet trains a LoRA adapter")
        return self.unet.lora
