"""The C2-shaped training step (bench.py's flagship: SDXL at 1024^2, LoRA r = 32, 2 pairs, gas 2, 8-bit AdamW) timed
on the bf16 library and on the f16 library, same box, same call.

    python tools/f16_step_bench.py [--steps 8] [--warmup 3] [--out profiles/f16_step.md]

The element type is per process, so each library runs in its own child process (PSO_LIB unset / PSO_LIB=f16) with its
own time limit; a child that fails or runs out of time ends the run.  Every step -- shuffle + one epoch + optimizer
step, exactly bench.py's one_step -- is bracketed by HIP events after a warm-up; the report gives the median, the
min-max spread (the run-to-run noise a difference has to exceed) and the f16 / bf16 ratio.  The f16 child trains with
dynamic loss scaling from 2^16 and reports how many optimizer steps the scaler skipped (a skipped step is shorter);
--loss-scale 0 runs it without the scaler, i.e. without the per-step read-back of the gradient norm."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(args):
    from types import SimpleNamespace
    import torch
    import pairwise_sample_optimization_amd as pkg
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    if not torch.cuda.is_available():
        raise SystemExit("f16_step_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    dt = pkg.compute_dtype()
    h = args.res // 8
    with torch.device(dev):
        unet = UNet2DConditionModel(UNetConfig.sdxl(h))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=args.rank, lora_alpha=args.rank))
    unet.lora.init_gaussian(seed=0, b_std=1e-3)
    unet.prepare()
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=args.gas,
                    train_batch_size=args.pairs, use_8bit_adam=True,
                    loss_scale=args.loss_scale if dt == torch.float16 and args.loss_scale > 0 else None)
    g = torch.Generator(device=dev).manual_seed(1000)
    Bp = args.pairs * args.gas
    enc = torch.randn(Bp, 77, 2048, device=dev, generator=g).to(dt)
    pooled = torch.randn(Bp, 1280, device=dev, generator=g).to(dt)
    tid = compute_time_ids(args.res, 0, dev).repeat(Bp, 1)
    buf = tr.sample_pairs(enc, pooled, tid, h, generator=g,
                          reward_fn=lambda img: torch.rand(img.shape[0], device=dev, generator=g))

    def step():
        tr.train_epoch(tr.shuffle(buf, generator=g))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    losses = [float(l) for l in tr.loss_hist[-4:]]
    print(json.dumps({"elem": str(dt), "step_ms": ms, "opt_steps": tr.opt_step,
                      "skipped": 0 if tr.scaler is None else tr.scaler.skipped,
                      "loss_scale": tr.loss_scale, "last_losses": losses,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def run_child(args, pso_lib):
    env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
    if pso_lib:
        env["PSO_LIB"] = pso_lib
    cmd = [sys.executable, "-u", os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--res", str(args.res), "--rank", str(args.rank), "--pairs", str(args.pairs), "--gas",
           str(args.gas), "--loss-scale", str(args.loss_scale)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"f16_step_bench: the {pso_lib or 'bf16'} child failed (rc={r.returncode})")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--gas", type=int, default=2)
    ap.add_argument("--loss-scale", type=float, default=65536.0,
                    help="initial loss scale of the f16 run; 0 = no scaler (no norm read-back: timing A/B only)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="write the markdown report here as well as to stdout")
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = [run_child(args, ""), run_child(args, "f16")]
    med = [statistics.median(r["step_ms"]) for r in res]
    lines = ["# fp16 vs bf16 training step", "",
             f"C2-shaped step on one {res[0]['device']}: SDXL UNet at {args.res}^2, LoRA r = {args.rank}, "
             f"{args.pairs} pairs x gas {args.gas} (= {2 * args.pairs * args.gas} images per step), 2-step turbo "
             f"sampler, 8-bit AdamW; shuffle + epoch + optimizer step between HIP events, {args.warmup} warm-up and "
             f"{args.steps} timed steps per library, each library in its own process, same call.", "",
             "| library | element | median ms | min ms | max ms | optimizer steps | skipped by the scaler |",
             "|---|---|---|---|---|---|---|"]
    for name, r, m in zip(("libpso_amd.so", "libpso_amd_f16.so"), res, med):
        lines.append(f"| {name} | {r['elem'].replace('torch.', '')} | {m:.2f} | {min(r['step_ms']):.2f} | "
                     f"{max(r['step_ms']):.2f} | {r['opt_steps']} | {r['skipped']} |")
    lines += ["", f"f16 / bf16 median ratio: {med[1] / med[0]:.4f}.  Final loss scale of the f16 run: "
              f"{res[1]['loss_scale']:g}.", ""]
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bf16_ms": med[0], "f16_ms": med[1], "ratio": med[1] / med[0], "runs": res}))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
