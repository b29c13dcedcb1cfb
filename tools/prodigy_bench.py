"""pso_prodigy_step against pso_adamw_step on one flat fp32 bucket, one process, same call, alternated.

    python tools/prodigy_bench.py [--n 46448640] [--rounds 3] [--reps 20] [--warmup 3] [--out FILE]

The default n is the r = 32 LoRA bucket of SDXL (46.45 M parameters).  A round times `reps` consecutive steps of one
optimizer between two device events, then the same of the other; the report gives the per-step time of every round
and the bandwidth each implies from the bytes the algorithm moves: AdamW 28 B per parameter (p, g, m, v read; p, m, v
written), Prodigy 52 B (pass 1: g, p, p0, m, v, s read and m, v, s written = 36; pass 2: p, m, v read and p written
= 16).  The gradient is a fixed seeded tensor; Prodigy runs with bias correction (its per-thread pow)."""
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
    ap.add_argument("--n", type=int, default=46_448_640)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    import torch
    from pairwise_sample_optimization_amd import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("prodigy_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    n = args.n
    gen = torch.Generator(device=dev).manual_seed(0)
    grad = torch.randn(n, device=dev, generator=gen)
    betas, eps, wd = (0.9, 0.999), 1e-8, 1e-2
    pa = 1e-2 * torch.randn(n, device=dev, generator=gen)
    pp = pa.clone()
    m, v = torch.zeros_like(pa), torch.zeros_like(pa)
    st = K.ProdigyState(pp, d0=1e-6)
    clip = K.grad_clip_coef(grad, 1.0)
    count = {"adamw": 0}

    def adamw():
        count["adamw"] += 1
        K.adamw_step(pa, grad, m, v, 1e-4, betas, eps, wd, count["adamw"], clip=clip)

    def prodigy():
        K.prodigy_step(pp, grad, st, 1.0, betas, eps, wd, use_bias_correction=True, safeguard_warmup=True, clip=clip)

    steps = {"adamw": adamw, "prodigy": prodigy}
    for fn in steps.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.reps)
    nbytes = {"adamw": 28.0 * n, "prodigy": 52.0 * n}
    sc = st.scalars()
    res = {"device": torch.cuda.get_device_name(0), "n": n, "reps": args.reps, "step_ms": ms,
           "median_ms": {k: statistics.median(x) for k, x in ms.items()},
           "bytes_per_step": nbytes,
           "tb_per_s": {k: nbytes[k] / (statistics.median(x) * 1e-3) / 1e12 for k, x in ms.items()},
           "prodigy_k": sc["k"], "prodigy_d_over_d0": sc["d"] / sc["d0"],
           "finite": bool(torch.isfinite(pp).all().item() and torch.isfinite(pa).all().item())}
    res["prodigy_over_adamw"] = res["median_ms"]["prodigy"] / res["median_ms"]["adamw"]
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
