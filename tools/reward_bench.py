"""Time of one PickScore reward call on the loaded library: full CLIP ViT-H/14 (vision 32 x 1280, text 24 x 1024,
synthetic weights) on 16 decoded images of 1024 x 1024 -- the reward of one bench.py epoch's sampling phase.

    python tools/reward_bench.py [--images 16] [--res 1024] [--calls 20] [--warmup 3] [--out FILE]
    PSO_LIB=f16 python tools/reward_bench.py ...          # the same on libpso_amd_f16.so (allow_f16=True)

The element type is per process, so the tool is run once per library; the images are of the library's element type in
[-1, 1], as the VAE decode leaves them.  A call is `Selector.score_tensor`: uint8 quantisation + PIL-exact resize +
vision tower + text tower + matched cosine.  Each call is timed on its own between two device events, after `warmup`
untimed calls; the report gives the median, the minimum and the maximum over the calls in milliseconds (the min-max
spread of the bf16 run is the noise a difference between the libraries has to exceed)."""
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
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="a 2-layer tower pair (a quick check of the tool itself)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reward_bench: no GPU (a timing needs one)")
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.clip import CLIPTextConfig, CLIPVisionConfig
    from pairwise_sample_optimization_amd.pso_pytorch.pickscore_utils import Selector
    dev = torch.device("cuda:0")
    tc, vc = CLIPTextConfig.pickscore_h(), CLIPVisionConfig()
    if args.tiny:
        tc.num_hidden_layers = vc.num_hidden_layers = 2
    sel = Selector(dev, seed=0, text_config=tc, vision_config=vc, allow_f16=True)
    g = torch.Generator(device=dev).manual_seed(0)
    n = args.images
    img = (0.6 * torch.randn(n, args.res, args.res, 3, device=dev, generator=g)).clamp(-1, 1)
    img = img.to(_lib.ELEM_DTYPE).contiguous()
    ids = torch.randint(1, 49406, (n, 77), device=dev, generator=g)
    ids[:, 0], ids[:, 20:] = 49406, 49407
    for _ in range(args.warmup):
        s = sel.score_tensor(img, ids)
    torch.cuda.synchronize()
    assert torch.isfinite(s).all()
    times = []
    for _ in range(args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sel.score_tensor(img, ids)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    res = {"library": os.path.basename(_lib.LIB_PATH), "elem": str(_lib.ELEM_DTYPE).replace("torch.", ""),
           "images": n, "res": args.res, "vision_layers": vc.num_hidden_layers, "text_layers": tc.num_hidden_layers,
           "calls": args.calls, "warmup": args.warmup, "unit": "ms per score_tensor call (device events)",
           "median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
