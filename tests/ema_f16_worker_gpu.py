"""Child process of tests/test_gpu_ema_f16.py (PSO_LIB=f16: the element type is per process): PSOTrainer with an
amp.DeviceLossScaler and use_ema.  Three optimizer steps on host-filled gradients, the second with one element set to
inf by a host-side fill -- pso_amp_unscale_clip rewrites the FOUND_INF word at every step from the gradient it reads,
so the word itself cannot be pre-set; no arithmetic on the device produces the inf.  On the skipped step the master
keeps its bits and the applied-step count stays, while the EMA's optimization_step advances and the shadow moves by
the restatement (tests/ema_ref.py) towards the unchanged master.  The steps run under
torch.cuda.set_sync_debug_mode("error"): nothing is read back."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import ema_ref
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    assert _lib.F16 and _lib.ELEM_DTYPE == torch.float16
    cuda = torch.device("cuda:0")
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    scaler = DeviceLossScaler(init_scale=1024.0, device=cuda)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, lr=1e-3, weight_decay=1e-2, loss_scale=scaler, use_ema=True,
                    ema_decay=0.9)
    master, grad = unet.lora.master, unet.lora.grad
    n = master.numel()
    # the gradients, made on the host: 3 x N(0, 1) times the loss scale; the second carries one inf
    hg = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=hg) * 3 * 1024.0 for _ in range(3)]
    grads[1][n - 1] = float("inf")
    grads = [g.to(cuda) for g in grads]
    torch.cuda.synchronize()
    probe = torch.ones(1, device=cuda)
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
        honoured = False
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want_decay = [0.0, 2 / 11, 3 / 12]
    for i in range(3):
        prev_shadow = tr.ema.shadow.cpu().numpy()
        prev_master = master.clone()
        grad.copy_(grads[i])
        torch.cuda.synchronize()
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            tr.optimizer_step()  # nothing is read back: a synchronising call would raise here
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert tr.ema.optimization_step == i + 1 and tr.ema.cur_decay_value == want_decay[i], (i, tr.ema.scalars())
        want = ema_ref.ema_update(prev_shadow, master.cpu().numpy(), ema_ref.one_minus_decay32(want_decay[i]))
        got = tr.ema.shadow.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), i
        if i == 1:  # the skipped step
            assert torch.equal(master.view(torch.int32), prev_master.view(torch.int32))
            assert tr.opt_step == 1 and scaler.skipped == 1 and scaler.scale == 512.0, scaler.state_dict()
            assert not np.array_equal(got, prev_shadow)  # the shadow still moved, towards the unchanged master
        else:
            assert not torch.equal(master, prev_master)
        assert grad.abs().max().item() == 0.0
    assert tr.opt_step == 2 and tr.ema.optimization_step == 3 and scaler.skipped == 1
    assert torch.isfinite(master).all() and torch.isfinite(tr.ema.shadow).all()
    assert torch.equal(unet.lora.work.view(torch.int16), master.half().view(torch.int16))
    print(f"EMA_F16_OK sync_debug={'on' if honoured else 'not honoured'} opt_step={tr.opt_step} "
          f"ema_step={tr.ema.optimization_step}", flush=True)


if __name__ == "__main__":
    main()
