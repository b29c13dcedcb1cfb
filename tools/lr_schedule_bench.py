"""Cost of the learning-rate schedule in the device-scaler optimizer step, one process, same call, alternated.

    python tools/lr_schedule_bench.py [--n 23500000] [--blocks 6] [--reps 1000] [--warmup 50] [--out FILE]

The device-scaler optimizer step of trainer.lora_optimizer_step on a flat fp32 buffer of n parameters (C2: LoRA r = 32
on SDXL is 23.5 M) with the 8-bit AdamW, as two launch sequences:
  fixed     pso_amp_unscale_clip -> pso_adamw8bit_step (amp_state, zero_grad, lr a host float) -> pso_amp_update
            -- what a trainer without a schedule launches, before and after the schedule existed
  schedule  pso_amp_unscale_clip -> pso_lr_schedule(amp_state) -> pso_adamw8bit_step (amp_state, zero_grad, lr_dev)
            -> pso_amp_update
Every repetition first refills the gradient from a fixed copy (the step zeroes it), in both sequences alike.  A block is
`reps` repetitions between two device events; blocks alternate fixed / schedule; the report gives the per-step median
and the min-max spread over the blocks of each, in microseconds.  The kernels are fp32 / integer: any library serves."""
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
    ap.add_argument("--n", type=int, default=23_500_000)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    import torch
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    if not torch.cuda.is_available():
        raise SystemExit("lr_schedule_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    n = args.n
    betas, eps, wd, lr = (0.9, 0.999), 1e-8, 1e-2, 1e-4
    gen = torch.Generator(device=dev).manual_seed(0)
    g0 = torch.randn(n, device=dev, generator=gen) * 1024.0 * 1e-3
    sched = LrSchedule("cosine", lr, 500, 1_000_000)
    runs = {}
    for name in ("fixed", "schedule"):
        p = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.02
        runs[name] = dict(p=p, grad=g0.clone(), work=K.cast_f32_bf16(p), st=K.Adam8State(n, dev, segments=[(0, n)]),
                          sc=DeviceLossScaler(init_scale=1024.0, device=dev), word=torch.zeros(1, device=dev),
                          times=[])

    def step(name):
        r = runs[name]
        sc = r["sc"]
        r["grad"].copy_(g0)
        K.amp_unscale_clip(r["grad"], 1.0, sc.state, betas)
        step_lr = lr
        if name == "schedule":
            step_lr = K.lr_schedule(sched, r["word"], amp_state=sc.state)
        K.adamw8bit_step(r["p"], r["grad"], r["st"], step_lr, betas, eps, wd, amp_state=sc.state, out_bf16=r["work"],
                         zero_grad=True)
        K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)

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
            runs[name]["times"].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    res = {"n": n, "reps": args.reps, "blocks": args.blocks, "unit": "us per optimizer step (incl. gradient refill)"}
    for name, r in runs.items():
        assert r["sc"].skipped == 0 and r["sc"].step == args.warmup + args.blocks * args.reps
        res[name] = {"median": round(statistics.median(r["times"]), 2), "min": round(min(r["times"]), 2),
                     "max": round(max(r["times"]), 2)}
    res["schedule_lr_word"] = runs["schedule"]["word"].item()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
