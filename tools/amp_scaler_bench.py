"""Host loss scaler against device loss scaler on the C2-shaped fp16 training step (SDXL at 1024^2, LoRA r = 32, 2 pairs,
gas 2, 8-bit AdamW, train_epoch_graph), one process, same call, alternated.

    PSO_LIB=f16 python tools/amp_scaler_bench.py [--blocks 6] [--block-steps 4] [--warmup 2] [--out FILE]

Two trainers share one UNet (and so one LoRA adapter); one trains with amp.LossScaler -- its optimizer step reads the
gradient norm back, and its captured epoch is keyed by the scale -- the other with amp.DeviceLossScaler.  A block is
`block-steps` consecutive steps (shuffle + graph epoch + optimizer step) of one trainer between two host-side
synchronisations, timed on the wall clock, so that the host trainer's per-step read-back shows as what it is: the end
of the CPU's run-ahead.  Blocks alternate host / device; the report gives the per-step median and the min-max spread
over the blocks of each.  Last, the scale of both is doubled and one more step is timed: the host trainer re-captures
its epoch, the device trainer replays the capture it has."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--block-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--gas", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    from types import SimpleNamespace
    import torch
    import pairwise_sample_optimization_amd as pkg
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler, LossScaler
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    if pkg.compute_dtype() != torch.float16:
        raise SystemExit("amp_scaler_bench: loss scaling is fp16 training -- run with PSO_LIB=f16")
    if not torch.cuda.is_available():
        raise SystemExit("amp_scaler_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    h = args.res // 8
    with torch.device(dev):
        unet = UNet2DConditionModel(UNetConfig.sdxl(h))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=args.rank, lora_alpha=args.rank))
    unet.lora.init_gaussian(seed=0, b_std=1e-3)
    unet.prepare()
    mk = lambda scaler: PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=args.gas,
                                   train_batch_size=args.pairs, use_8bit_adam=True, loss_scale=scaler)
    trainers = {"host": mk(LossScaler()), "device": mk(DeviceLossScaler(device=dev))}
    g = torch.Generator(device=dev).manual_seed(1000)
    Bp = args.pairs * args.gas
    enc = torch.randn(Bp, 77, 2048, device=dev, generator=g).half()
    pooled = torch.randn(Bp, 1280, device=dev, generator=g).half()
    tid = compute_time_ids(args.res, 0, dev).repeat(Bp, 1)
    buf = trainers["host"].sample_pairs(enc, pooled, tid, h, generator=g,
                                        reward_fn=lambda img: torch.rand(img.shape[0], device=dev, generator=g))

    def step(tr):
        tr.train_epoch_graph(tr.shuffle(buf, generator=g))

    def block(tr, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for tr in trainers.values():
        for _ in range(args.warmup):  # the first call captures
            step(tr)
    ms = {k: [] for k in trainers}
    for _ in range(args.blocks):
        for k, tr in trainers.items():
            ms[k].append(block(tr, args.block_steps))
    graphs = {k: tr._graph for k, tr in trainers.items()}
    change = {}
    for k, tr in trainers.items():
        tr.scaler.scale = tr.scaler.scale * 2.0
        change[k] = block(tr, 1)
    res = {"device": torch.cuda.get_device_name(0), "block_steps": args.block_steps,
           "step_ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()},
           "min_ms": {k: min(v) for k, v in ms.items()}, "max_ms": {k: max(v) for k, v in ms.items()},
           "step_after_scale_change_ms": change,
           "recaptured": {k: trainers[k]._graph is not graphs[k] for k in trainers},
           "opt_steps": {k: tr.opt_step for k, tr in trainers.items()},
           "skipped": {k: tr.scaler.skipped for k, tr in trainers.items()},
           "loss_scale": {k: tr.loss_scale for k, tr in trainers.items()}}
    res["device_over_host"] = res["median_ms"]["device"] / res["median_ms"]["host"]
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
