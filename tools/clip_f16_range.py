"""Activation range of the CLIP towers under the f16 library, for a local checkpoint: each encoder layer's largest
|activation| against fp16's largest finite value, 65504.

    PSO_LIB=f16 python tools/clip_f16_range.py PATH [--kind clip|text|text_proj] [--subfolder NAME]
                                               [--tokenizer DIR --prompt "..." ...] [--images 4] [--res 512]

PATH is a transformers directory (config.json + model.safetensors / pytorch_model.bin): a CLIPModel such as PickScore_v1
(--kind clip, the default: both towers run), or an SDXL text encoder (--kind text with --subfolder text_encoder,
--kind text_proj with --subfolder text_encoder_2).  Prompts are tokenized when --tokenizer names a local tokenizer
directory; otherwise random token ids stand in (bos, 18 tokens, eos padding).  Images are random, N(0, 0.6) clamped to
[-1, 1]: pass real decoded images through the library to look at a particular case.

The largest |value| per layer is taken over every tensor the layer forms: the two LayerNorm outputs, q/k/v, the
attention output, the MLP's fc1 output before and after the activation, and the residual stream after each of the
two blocks.  An `inf` or a value near 65504 means the checkpoint does not fit fp16 at that layer: use the bf16 library
for that model.  The towers' fp16 headroom with trained weights has not been verified by the project itself (no
checkpoint is available to its tests); this tool is how a user with the weights looks."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F16_MAX = 65504.0


class Recorder:
    """Wraps the kernels.py calls clip.py makes, keeping the largest |value| of every tensor they return."""
    NAMES = ("gemm", "attention_small", "layer_norm_fwd", "activation_", "embed_tokens", "embed_vision")

    def __init__(self, K):
        self.K, self.saved, self.peak = K, {}, 0.0

    def _wrap(self, fn):
        def call(*a, **kw):
            out = fn(*a, **kw)
            t = out[0] if isinstance(out, tuple) else out
            self.peak = max(self.peak, float(t.float().abs().max()))  # inf / nan stay visible
            return out
        return call

    def __enter__(self):
        for n in self.NAMES:
            self.saved[n] = getattr(self.K, n)
            setattr(self.K, n, self._wrap(self.saved[n]))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.K, n, fn)

    def take(self):
        p, self.peak = self.peak, 0.0
        return p


def trace_tower(name, tower, run, rec):
    """Runs `run()` with every encoder layer's fwd wrapped; prints one line per stage."""
    rows = []
    for i, layer in enumerate(tower.encoder.layers):
        def fwd(*a, _f=layer.fwd, _i=i, **kw):
            rows.append(("embeddings" if _i == 0 else f"between {_i - 1} and {_i}", rec.take()))
            out = _f(*a, **kw)
            rows.append((f"layer {_i}", rec.take()))
            return out
        layer.fwd = fwd
    try:
        out = run()
    finally:
        for layer in tower.encoder.layers:
            del layer.fwd
    rows.append(("after the last layer", rec.take()))
    print(f"{name}: largest |activation| per stage (fp16 max {F16_MAX:.0f})")
    worst = 0.0
    for what, peak in rows:
        if what.startswith("between") and peak == 0.0:
            continue
        worst = max(worst, peak) if peak == peak else float("nan")
        print(f"  {what:24s} {peak:12.4g}   {peak / F16_MAX * 100:8.3f} % of the fp16 range")
    print(f"  {name} worst: {worst:.4g} ({worst / F16_MAX * 100:.3f} %)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--kind", default="clip", choices=["clip", "text", "text_proj"])
    ap.add_argument("--subfolder", default=None)
    ap.add_argument("--tokenizer", default=None, help="local tokenizer directory (for --prompt)")
    ap.add_argument("--prompt", action="append", default=None)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--res", type=int, default=512)
    args = ap.parse_args()
    import torch
    from pairwise_sample_optimization_amd import _lib
    if not _lib.F16:
        raise SystemExit("clip_f16_range: run with PSO_LIB=f16 (the range in question is the f16 library's)")
    if not torch.cuda.is_available():
        raise SystemExit("clip_f16_range: no GPU (the towers run on the HIP kernels only)")
    from pairwise_sample_optimization_amd import clip
    from pairwise_sample_optimization_amd import kernels as K
    dev = torch.device("cuda:0")
    cls = {"clip": clip.CLIPModel, "text": clip.CLIPTextModel, "text_proj": clip.CLIPTextModelWithProjection}[args.kind]
    m = cls.from_pretrained(args.path, subfolder=args.subfolder, allow_f16=True).to(dev)
    lost = [k for k, v in m.state_dict().items() if not torch.isfinite(v).all()]
    print(f"{args.path}: {len(lost)} tensors with values outside the fp16 range after the cast" +
          (f": {lost[:8]}" if lost else ""))
    tcfg = m.text_config if args.kind == "clip" else m.config
    g = torch.Generator(device=dev).manual_seed(0)
    if args.prompt and args.tokenizer:
        from pairwise_sample_optimization_amd.prompts import load_tokenizer
        tok = load_tokenizer(args.tokenizer)
        ids = tok(args.prompt, padding="max_length", truncation=True, max_length=tcfg.max_position_embeddings,
                  return_tensors="pt").input_ids.to(dev)
    else:
        n = len(args.prompt) if args.prompt else 4
        ids = torch.randint(1, tcfg.vocab_size - 2, (n, tcfg.max_position_embeddings), device=dev, generator=g)
        ids[:, 0], ids[:, 20:] = tcfg.vocab_size - 2, tcfg.vocab_size - 1
    m._ensure()
    with torch.no_grad(), Recorder(K) as rec:
        trace_tower("text tower", m.text_model, lambda: m.text_model.fwd(ids), rec)
        if args.kind == "clip":
            img = (0.6 * torch.randn(args.images, args.res, args.res, 3, device=dev, generator=g)).clamp(-1, 1)
            feats = trace_tower("vision tower", m.vision_model,
                                lambda: m.image_features_from_images(img.half().contiguous()), rec)
            print(f"image features finite: {bool(torch.isfinite(feats).all())}")


if __name__ == "__main__":
    main()
