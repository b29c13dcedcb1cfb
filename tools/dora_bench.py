"""Cost of DoRA on the flagship training step, one process, alternated.

    python tools/dora_bench.py [--res 1024] [--rank 32] [--pairs 2] [--gas 2] [--blocks 6] [--reps 2] [--warmup 2]
                               [--out FILE]

Two SDXL UNets with the same frozen weights and the same LoRA A / B -- one a plain LoRA adapter, one a DoRA adapter
(use_dora) -- each under a PSOTrainer set up as bench.py's C2 step (1024 x 1024, rank 32, 2 pairs, 8-bit AdamW): a step
is shuffle + train_epoch, i.e. gas paired micro-steps and one optimizer step (for DoRA that includes the row-norm
launch of refresh()).  A block is `reps` steps between two device events; blocks alternate lora / dora; the report
gives the per-step median and the min-max spread over the blocks of each, in milliseconds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--gas", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiny", action="store_true", help="the tiny topology (a quick check of the tool itself)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    from types import SimpleNamespace
    import torch
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    if not torch.cuda.is_available():
        raise SystemExit("dora_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    h = args.res // 8
    cfg = UNetConfig.tiny(h) if args.tiny else UNetConfig.sdxl(h)
    runs = {}
    for name in ("lora", "dora"):
        with torch.device(dev):
            unet = UNet2DConditionModel(cfg)
        unet.init_weights(0)
        unet.add_adapter(SimpleNamespace(r=args.rank, lora_alpha=args.rank, use_dora=name == "dora"), allow_dora=True)
        unet.lora.init_gaussian(seed=0, b_std=1e-3)
        unet.prepare()
        tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=args.gas,
                        train_batch_size=args.pairs, num_reward=1, use_8bit_adam=True)
        g = torch.Generator(device=dev).manual_seed(1000)
        Bp = args.pairs * args.gas
        enc = torch.randn(Bp, 77, cfg.cross_attention_dim, device=dev, generator=g).bfloat16()
        pooled = torch.randn(Bp, cfg.text_embed_dim, device=dev, generator=g).bfloat16()
        tid = compute_time_ids(args.res, 0, dev).repeat(Bp, 1)
        buf = tr.sample_pairs(enc, pooled, tid, h, generator=g,
                              reward_fn=lambda img: torch.rand(img.shape[0], device=dev, generator=g))
        runs[name] = dict(unet=unet, tr=tr, buf=buf, g=g, times=[])

    def step(name):
        r = runs[name]
        r["tr"].train_epoch(r["tr"].shuffle(r["buf"], generator=r["g"]))

    for name in runs:
        for _ in range(args.warmup):
            step(name)
    torch.cuda.synchronize()
    for _ in range(args.blocks):
        for name in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                step(name)
            e1.record()
            torch.cuda.synchronize()
            runs[name]["times"].append(e0.elapsed_time(e1) / args.reps)
    res = {"res": args.res, "rank": args.rank, "pairs": args.pairs, "gas": args.gas, "reps": args.reps,
           "blocks": args.blocks, "unit": "ms per step (shuffle + gas paired micro-steps + optimizer step)"}
    for name, r in runs.items():
        assert torch.isfinite(r["unet"].lora.master).all()
        res[name] = {"median": round(statistics.median(r["times"]), 2), "min": round(min(r["times"]), 2),
                     "max": round(max(r["times"]), 2)}
    res["dora_over_lora"] = round(res["dora"]["median"] / res["lora"]["median"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
