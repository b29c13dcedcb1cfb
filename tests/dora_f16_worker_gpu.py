"""Child process of tests/test_gpu_dora_f16.py (PSO_LIB=f16: the element type is per process): the tiny16 DoRA parity
case of tests/test_gpu_dora.py on the fp16 library, its backward run on the loss times a host amp.LossScaler's scale
(1024) and the gradients unscaled, at the same bars."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import dora_ref
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.amp import LossScaler
    assert _lib.F16 and _lib.ELEM_DTYPE == torch.float16
    scaler = LossScaler(init_scale=1024.0)
    c = dora_ref.gpu_parity_case("tiny16", 8, loss_scale=scaler.scale)
    assert c.unet.lora.work.dtype == torch.float16 and c.unet.lora.dora
    assert c.moved_eps >= 3 * dora_ref.FWD_BAR and c.moved_grad >= 10 * dora_ref.GRAD_BAR, (c.moved_eps, c.moved_grad)
    assert set(c.mine) == set(c.ref) and len(c.mkeys) * 3 == len(c.ref)
    assert torch.isfinite(c.out).all() and all(torch.isfinite(v).all() for v in c.mine.values())
    assert c.dora_eps < dora_ref.FWD_BAR, c.dora_eps
    assert c.dora_grad < dora_ref.GRAD_BAR, c.dora_grad
    assert c.mag_grad < dora_ref.GRAD_BAR, c.mag_grad
    print(f"DORA_F16_OK eps={c.dora_eps:.3e} grads={c.dora_grad:.3e} magnitudes={c.mag_grad:.3e}", flush=True)


if __name__ == "__main__":
    main()
