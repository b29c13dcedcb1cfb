"""World-1 RCCL rank of tests/test_gpu_lora_narrow_rank.py::test_overlapped_sync_equals_flat_sync_world1 (the world-1
case of tests/rccl_worker_gpu.py at LoRA rank 4 on the tiny UNet; started directly, the rendezvous is a file store).

Rank-4 adapters run their weight-gradient products into the padded scratch on the side stream (PSO_SIDE_STREAM path,
products not batched); each gradient unit's fold follows them there, and GradBuckets joins the side stream before the
unit's bucket leaves.  One optimizer step with the overlapped bucketed sync against one with the flat post-backward
all-reduce from the same initial weights: equal synced gradients and equal masters, bit for bit.
Writes rank0.json into --out."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method="file://" + os.path.join(os.path.abspath(args.out), "rendezvous"),
                            rank=0, world_size=1, device_id=dev)
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd import unet as unet_mod
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    K.SideStream.enabled = True   # weight-gradient closures and the folds on the side stream ...
    unet_mod.TN_BATCH = False     # ... and nothing deferred to the compute stream
    cfg = UNetConfig.tiny(16)
    elem = _lib.ELEM_DTYPE

    def make(overlap):
        with torch.device(dev):
            u = UNet2DConditionModel(cfg)
        u.init_weights(0)
        u.add_adapter(SimpleNamespace(r=4, lora_alpha=4))
        u.lora.init_gaussian(seed=1, b_std=0.05)
        u.prepare()
        # 8 kB buckets: every attention unit of the tiny UNet (32 kB of rank-4 gradient per block) is its own bucket
        t = PSOTrainer(u, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, lr=1e-3,
                       overlap_sync=overlap, bucket_mb=8.0 / 1024, loss_scale=256.0 if _lib.F16 else None)
        return u, t

    unet, tr = make(True)
    g = torch.Generator(device="cuda").manual_seed(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=dev, generator=g).to(elem)
    pooled = torch.randn(1, cfg.text_embed_dim, device=dev, generator=g).to(elem)
    tid = compute_time_ids(128, 0, dev)
    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=dev, generator=g))
    sb = tr.shuffle(buf, generator=torch.Generator(device="cuda").manual_seed(100))
    mb = tr.micro_batch(sb, 0, sb.n_micro)
    st = unet.lora
    grads = {}
    step = tr.optimizer_step

    def grab_then_step():
        grads["issued"] = sum(w is not None for w in tr.buckets.works)
        tr.buckets.finish()
        tr.sync_armed = False
        grads["a"] = st.grad.clone()
        grads["scratch_a"] = bool((st.grad_pad == 0).all())
        step()
    tr.optimizer_step = grab_then_step
    tr.micro_step(mb)
    torch.cuda.synchronize()
    ma = st.master.clone()

    unet2, tr2 = make(False)
    st2 = unet2.lora
    step2 = tr2.optimizer_step

    def grab_flat_then_step():
        grads["b"] = st2.grad.clone()
        grads["scratch_b"] = bool((st2.grad_pad == 0).all())
        step2()  # the flat all-reduce of lora_optimizer_step
    tr2.optimizer_step = grab_flat_then_step
    tr2.micro_step(mb)
    torch.cuda.synchronize()
    mb_ = st2.master.clone()
    ga, gb = grads["a"], grads["b"]
    res = dict(backend=dist.get_backend(), world=dist.get_world_size(), rank=st.r, buckets=len(tr.buckets.buckets),
               issued_before_finish=grads["issued"], grad_norm=ga.norm().item(),
               bucketed_equals_flat=bool(torch.equal(ga, gb)), masters_equal=bool(torch.equal(ma, mb_)),
               scratch_zero=bool(grads["scratch_a"] and grads["scratch_b"]))
    with open(os.path.join(args.out, "rank0.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
