"""Child process of tests/test_gpu_prodigy.py::test_prodigy_trains_on_the_f16_library (PSO_LIB=f16: the element type is
per process): one accumulation window of PSOTrainer(optimizer="prodigy") with an amp.DeviceLossScaler -- the scaler's
block feeds the Prodigy step its gradient factor and inf-skip -- then the state is read back once."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    assert _lib.F16 and _lib.ELEM_DTYPE == torch.float16
    cuda = torch.device("cuda:0")
    cfg = UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    scaler = DeviceLossScaler(init_scale=1024.0, device=cuda)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, lr=1.0,
                    optimizer="prodigy", loss_scale=scaler)
    g = torch.Generator(device="cuda").manual_seed(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).half()
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).half()
    buf = tr.sample_pairs(enc, pooled, compute_time_ids(128, 0, cuda), 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    sb = tr.shuffle(buf, generator=torch.Generator(device="cuda").manual_seed(100))
    master0 = unet.lora.master.clone()
    tr.train_epoch(sb)
    torch.cuda.synchronize()
    sc = tr.prodigy.scalars()
    assert tr.opt_step == 1 and scaler.skipped == 0 and scaler.scale == 1024.0, (tr.opt_step, scaler.state_dict())
    assert sc["updated"] == 1 and sc["skipped"] == 0 and sc["dlr"] > 0, sc
    assert torch.isfinite(unet.lora.master).all() and not torch.equal(unet.lora.master, master0)
    assert unet.lora.grad.abs().max().item() == 0.0
    assert torch.equal(unet.lora.work.view(torch.int16), unet.lora.master.half().view(torch.int16))
    print(f"PRODIGY_F16_OK k={sc['k']}", flush=True)


if __name__ == "__main__":
    main()
