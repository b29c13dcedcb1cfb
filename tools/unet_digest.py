"""Bit digests of the UNet forward / backward in every adapter mode: sha256 of eps and of every LoRA / magnitude / full
gradient, for comparing two commits bit for bit (a refactor of unet.py must leave every line unchanged).

    python -m tools.unet_digest [--verbose] [mode ...]

Prints one line per mode: eps digest, the number of gradient tensors and one digest over their (name, sha256) list
(--verbose: every tensor's own).  Run it twice on the old commit first: a mode whose lines differ between those two
runs is not bit-stable and tells nothing.  The adapters start from init_gaussian(b_std > 0) with the DoRA magnitudes
moved away from m = n (with B = 0 merged and base weights are bit-equal and a wrong operand would not show), and the
backward takes a fixed non-zero dout.

MODES / build() / run() are also what tests/test_gpu_unet_launch_trace.py records its launch sequences from."""
import hashlib
import sys
from types import SimpleNamespace

import torch

# the smallest UNet whose transformer widths the e4m3 GEMM takes (N % 256 == 0, K % 128 == 0)
FP8_WIDTHS = dict(block_out_channels=(64, 256, 256), transformer_layers_per_block=(1, 1, 1), cross_attention_dim=128,
                  addition_time_embed_dim=32, text_embed_dim=64, time_proj_dim=64, sample_size=16)
FP8_ALL = ("qkv", "q2", "ff", "ffout", "out", "tail")

# name -> r (0: no adapter), and what the pass does.  fp8: the FP8_KINDS of the pass (FP8_MIN_TILES = 0 and
# FP8_ROUND_GAIN = 1e9 lift the occupancy rules, as tests/test_gpu_fp8.py does)
MODES = {
    "lora_r8": dict(r=8, backward=True),
    "paired_r8": dict(r=8, paired=True, backward=True),
    "adapters_off": dict(r=8, disabled=True),
    "paired_r4": dict(r=4, paired=True, backward=True),
    "paired_dora": dict(r=8, dora=True, paired=True, backward=True),
    "fused": dict(r=8, fused=True),
    "full_grad": dict(r=0, full=True, backward=True),
    "fp8_paired_r16": dict(r=16, paired=True, backward=True, fp8=("q2", "ff", "tail")),
    # no "tail": qkv / q2 take the bf16 LoRA term (diagnostic form), o1 / o2 the e4m3 tail all the same
    "fp8_no_tail_r16": dict(r=16, paired=True, backward=True, fp8=("qkv", "q2", "ff", "out")),
    "fp8_all_r16": dict(r=16, paired=True, backward=True, fp8=FP8_ALL),
    "fp8_all_off": dict(r=16, disabled=True, fp8=FP8_ALL),
}


def build(name, dev):
    """(unet, inputs) of mode `name`, prepared: the first recorded call is the forward's first launch."""
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    m = MODES[name]
    cfg = UNetConfig(**FP8_WIDTHS) if m.get("fp8") else UNetConfig.tiny(16)
    unet = UNet2DConditionModel(cfg).init_weights(0).to(dev)
    if m.get("full"):
        unet.enable_full_grads()
    if m["r"]:
        st = unet.add_adapter(SimpleNamespace(r=m["r"], lora_alpha=m["r"], use_dora=bool(m.get("dora"))),
                              allow_dora=True)
        st.init_gaussian(seed=1, b_std=0.05)
        if m.get("dora"):
            st.init_magnitudes()
            gen = torch.Generator().manual_seed(7)
            for nm in st.adapter_names():
                mag = st.magnitude_view(st.master, nm)
                mag.mul_((0.75 + 0.5 * torch.rand(mag.shape, generator=gen)).to(dev))
            st.refresh()
    unet.prepare()
    if m.get("fp8"):
        unet.enable_fp8_forward()
    if m.get("fused"):
        unet.fuse_lora()
    if m.get("disabled"):
        unet.disable_adapters()
    g = torch.Generator().manual_seed(3)
    h = cfg.sample_size
    x = K.nchw_to_nhwc(torch.randn(1, 4, h, h, generator=g).to(dev))
    inp = SimpleNamespace(x=x, t=torch.tensor([499.0], device=dev),
                          enc=torch.randn(1, 77, cfg.cross_attention_dim, generator=g).bfloat16().to(dev),
                          text=torch.randn(1, cfg.text_embed_dim, generator=g).bfloat16().to(dev),
                          tid=torch.tensor([[8 * h, 8 * h, 0, 0, 8 * h, 8 * h]], device=dev, dtype=torch.float32),
                          dout=torch.randn(1, h, h, 4, generator=g).to(x.dtype).to(dev))
    return unet, inp


def run(name, unet, inp):
    """One forward_nhwc (+ backward_nhwc) of mode `name`; returns (eps, {gradient name: tensor})."""
    from pairwise_sample_optimization_amd import unet as U
    m = MODES[name]
    saved = U.FP8_KINDS, U.FP8_MIN_TILES, U.FP8_ROUND_GAIN
    if m.get("fp8"):
        U.FP8_KINDS, U.FP8_MIN_TILES, U.FP8_ROUND_GAIN = set(m["fp8"]), 0, 1e9
    try:
        bwd = bool(m.get("backward"))
        eps, rt = unet.forward_nhwc(inp.x, inp.t, inp.enc, inp.text, inp.tid, save=bwd,
                                    paired_ref=bool(m.get("paired")))
        grads = {}
        if bwd:
            unet.backward_nhwc(inp.dout, rt)
            if m.get("full"):
                grads = {n: unet.full.g(p) for n, p in unet.named_parameters()}
            else:
                grads = unet.lora.grad_dict_peft()
    finally:
        U.FP8_KINDS, U.FP8_MIN_TILES, U.FP8_ROUND_GAIN = saved
    return eps, grads


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def main(argv):
    verbose = "--verbose" in argv
    names = [a for a in argv if not a.startswith("--")] or list(MODES)
    dev = torch.device("cuda:0")
    for name in names:
        unet, inp = build(name, dev)
        eps, grads = run(name, unet, inp)
        torch.cuda.synchronize()
        per = sorted((k, sha(v)) for k, v in grads.items())
        allg = hashlib.sha256(repr(per).encode()).hexdigest() if per else "-"
        print(f"{name}: eps {sha(eps)} grads[{len(per)}] {allg}", flush=True)
        if verbose:
            for k, d in per:
                print(f"    {d} {k}")
        del unet, inp, eps, grads


if __name__ == "__main__":
    main(sys.argv[1:])
