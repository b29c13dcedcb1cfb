"""What fuse_lora() buys on the no-grad forward, one process, alternated; and what the merge launch costs.

    python tools/fuse_bench.py [--res 1024] [--rank 32] [--images 2,16] [--blocks 6] [--reps 2] [--warmup 2]
                               [--merges 5] [--out FILE]

One SDXL UNet per adapter kind -- a plain LoRA adapter, then a DoRA adapter (use_dora) -- with B != 0.  For each batch
size in --images the no-grad forward (the sampling forward of a PSO epoch: forward_nhwc(save=False)) is timed on the
adapter path and on the merged weights: a block is `reps` forwards between two device events; blocks alternate
adapter / fused (fuse_lora() / unfuse_lora() between them launch nothing: the adapter version does not change); the
report gives the per-forward median and the min-max spread over the blocks of each side, in milliseconds, and the eps
difference between the two paths.  `merge`: the pso_lora_merge launch alone (all adapted projections of the UNet),
between device events."""
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
    ap.add_argument("--images", default="2,16", help="comma-separated batch sizes of the timed forward")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--merges", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the tiny topology (a quick check of the tool itself)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    if args.blocks < 6:
        raise SystemExit("fuse_bench: at least six blocks per side")
    from types import SimpleNamespace
    import torch
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    if not torch.cuda.is_available():
        raise SystemExit("fuse_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    h = args.res // 8
    cfg = UNetConfig.tiny(h) if args.tiny else UNetConfig.sdxl(h)
    sizes = [int(n) for n in args.images.split(",")]
    res = {"res": args.res, "rank": args.rank, "reps": args.reps, "blocks": args.blocks,
           "unit": "ms per no-grad forward (median, min, max over the blocks of a side)"}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(ts):
        return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    for kind in ("lora", "dora"):
        with torch.device(dev):
            unet = UNet2DConditionModel(cfg)
        unet.init_weights(0)
        unet.add_adapter(SimpleNamespace(r=args.rank, lora_alpha=args.rank, use_dora=kind == "dora"), allow_dora=True)
        unet.lora.init_gaussian(seed=0, b_std=1e-3)
        unet.prepare()
        unet.fuse_lora()
        merged = sum(t.numel() for b in unet._merged.blk.values() for t in vars(b).values()) + \
            sum(t.numel() for t in unet._merged.kv.values())
        out = {"merged_elements": merged, "merged_bytes": merged * 2}
        for _ in range(args.warmup):
            unet.lora.merge()
        torch.cuda.synchronize()
        out["merge"] = stats([timed(unet.lora.merge, 1) for _ in range(args.merges)])
        for n in sizes:
            g = torch.Generator(device=dev).manual_seed(1000 + n)
            x = torch.randn(n, h, h, 4, device=dev, generator=g).to(K.ELEM)
            t = torch.full((n,), 999.0, device=dev)
            enc = torch.randn(n, 77, cfg.cross_attention_dim, device=dev, generator=g).to(K.ELEM)
            pooled = torch.randn(n, cfg.text_embed_dim, device=dev, generator=g).to(K.ELEM)
            tid = compute_time_ids(args.res, 0, dev).repeat(n, 1)

            def fwd():
                with torch.no_grad():
                    return unet.forward_nhwc(x, t, enc, pooled, tid, save=False)[0]

            sides = {"adapter": unet.unfuse_lora, "fused": unet.fuse_lora}
            eps, times = {}, {k: [] for k in sides}
            for name, switch in sides.items():
                switch()
                for _ in range(args.warmup):
                    eps[name] = fwd()
            torch.cuda.synchronize()
            ver = unet.lora.merge_version
            for _ in range(args.blocks):
                for name, switch in sides.items():
                    switch()
                    times[name].append(timed(fwd, args.reps))
            assert unet.lora.merge_version == ver == unet.lora.version, "the timed blocks must not re-merge"
            assert torch.isfinite(eps["fused"].float()).all()
            diff = ((eps["fused"].float() - eps["adapter"].float()).norm() / eps["adapter"].float().norm()).item()
            out[f"images_{n}"] = {"adapter": stats(times["adapter"]), "fused": stats(times["fused"]),
                                  "fused_over_adapter": round(statistics.median(times["fused"]) /
                                                              statistics.median(times["adapter"]), 4),
                                  "eps_rel_diff": float(f"{diff:.3e}")}
        res[kind] = out
        del unet
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
