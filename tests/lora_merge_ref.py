"""fp64 restatement of the merged LoRA / DoRA weight and the error bound that goes with it, in plain torch and sharing
no code with the product (csrc/lora_merge.hip, kernels.LoraMergeTable).

    ref64[j][i] = g_j ( W[j][i] + s sum_k B[j][k] A[k][i] )                     (g absent: 1)
    |got - ref64| <= 1/2 ulp16(ref64) + (r + 3) 2^-24 |g_j| ( |W_ji| + |s| sum_k |B_jk A_ki| )

The first term is the one rounding to the 16-bit element type.  The second is the standard fp32 bound for what precedes
it: r multiply-adds (fused or not: each costs at most one unit roundoff 2^-24 relative to the running sum of absolute
values), the product by s, the add of W and the product by g -- r + 3 roundings, each bounded against the sum of the
absolute values of the terms.  It is derived, not tuned: nothing in it comes from what the kernel returns.  (The fp32
value may fall in the binade above ref64's, where the 16-bit ulp doubles; the power of two between them is
representable, so the total still stays below the sum of the two terms.)
"""
import torch

# explicit mantissa bits / smallest normal exponent of the 16-bit element types
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def ulp16(x, dtype):
    """One unit in the last place of `dtype` at the magnitude of the fp64 values x (the subnormal spacing below the
    smallest normal)."""
    bits, emin = _FMT[dtype]
    _, e = torch.frexp(x.abs().double())          # |x| = f 2^e, f in [0.5, 1): the binade is 2^(e-1)
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)  # frexp(0) has exponent 0
    return torch.exp2((e - bits).double())


def merged64(W, A, B, s, g=None):
    """The merged weight in fp64 from the 16-bit-valued W [out, in] and the fp32 A [r, in], B [out, r], g [out]."""
    m = W.double() + float(s) * (B.double() @ A.double())
    return m if g is None else g.double()[:, None] * m


def bound(W, A, B, s, g, dtype):
    """The elementwise bound above for a merge into `dtype`."""
    ref = merged64(W, A, B, s, g)
    mag = W.double().abs() + abs(float(s)) * (B.double().abs() @ A.double().abs())
    if g is not None:
        mag = g.double().abs()[:, None] * mag
    return 0.5 * ulp16(ref, dtype) + (A.shape[0] + 3) * 2.0 ** -24 * mag


def worst(got, W, A, B, s, g, dtype):
    """max |got - ref64| / bound over the elements (<= 1 passes), and the number of elements above it."""
    ratio = (got.double() - merged64(W, A, B, s, g)).abs() / bound(W, A, B, s, g, dtype)
    return ratio.max().item(), int((ratio > 1).sum())


# ----------------------------------------------------------------------------------------------------------------------
# GPU cases shared by tests/test_gpu_lora_merge.py and tests/lora_merge_f16_worker_gpu.py
# ----------------------------------------------------------------------------------------------------------------------
# (out, in, r): fewer rows than one wave's group and one partial lane sweep; the 256-column sweep boundary with a
# 4-column remainder and rows that are no multiple of the block's 16; the middle third of a q / k / v stack into the
# middle third of a wider buffer; the cross-attention k / v class; a rank above 32
SHAPES = [(5, 8, 1), (19, 260, 4), (64, 320, 8), (33, 2048, 32), (8, 64, 40)]
STACKED = (64, 320, 8)
SENTINEL = 0x7FA5  # a NaN with a payload: no computed value has these bits


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def kernel_operands(shape, use_g, cuda, seed=0):
    """Random 16-bit-valued W and fp32 A, B (and g) of one record, with a destination whose surroundings can be
    checked afterwards: returns a namespace with W, A, B, g, O and untouched(), which asserts that nothing outside O
    was written.  The STACKED shape reads W as rows 64..127 of a [192, 320] stack and writes O as rows 64..127,
    columns 0..319 of a [192, 328] buffer; the others write into a parity_util.guarded buffer."""
    from types import SimpleNamespace
    import parity_util as P
    from pairwise_sample_optimization_amd import kernels as K
    out, fin, r = shape
    g0 = torch.Generator(device="cuda").manual_seed(1000 * seed + out + fin + r)
    c = SimpleNamespace(shape=shape)
    c.A = torch.randn(r, fin, device=cuda, generator=g0) / r
    c.B = torch.randn(out, r, device=cuda, generator=g0) * 0.1
    c.g = torch.exp2(torch.rand(out, device=cuda, generator=g0) * 2 - 1) if use_g else None
    if shape == STACKED:
        stack = (torch.randn(3 * out, fin, device=cuda, generator=g0) * fin ** -0.5).to(K.ELEM)
        c.W = stack[out:2 * out]
        buf = torch.empty(3 * out, fin + 8, device=cuda, dtype=K.ELEM)
        buf.view(torch.int16).fill_(SENTINEL)
        c.O = buf[out:2 * out, :fin]

        def untouched(what="pso_lora_merge"):
            keep = buf.view(torch.int16) == SENTINEL
            assert keep[:out].all() and keep[2 * out:].all(), f"{what}: rows outside the middle third were written"
            assert keep[:, fin:].all(), f"{what}: the 8 gap columns were written"
            assert not keep[out:2 * out, :fin].any(), f"{what}: destination elements were left unwritten"
    else:
        c.W = (torch.randn(out, fin, device=cuda, generator=g0) * fin ** -0.5).to(K.ELEM)
        (c.O,), check = P.guarded(out, [fin], device=cuda)

        def untouched(what="pso_lora_merge"):
            check(what)
            assert not (bits(c.O) == SENTINEL).any(), f"{what}: destination elements were left unwritten"
    c.untouched = untouched
    return c


def run_merge(cases, s, cuda):
    """One pso_lora_merge launch over the records `cases` at scale s."""
    from pairwise_sample_optimization_amd import kernels as K
    K.LoraMergeTable([(c.W, c.A, c.B, s, c.g, c.O) for c in cases], cuda).run()
    torch.cuda.synchronize()


def check_bound(c, s, tag):
    from pairwise_sample_optimization_amd import kernels as K
    c.untouched(tag)
    w, over = worst(c.O, c.W, c.A, c.B, s, c.g, K.ELEM)
    print(f"  {tag}: max |got - ref64| / bound = {w:.3f}", flush=True)
    assert torch.isfinite(c.O.float()).all() and over == 0 and w <= 1.0, (tag, w, over)


def kernel_bound_cases(cuda):
    """Every shape alone and all five as one launch, with and without g, at s = 0.5 and s = 0.35."""
    for use_g in (False, True):
        for s in (0.5, 0.35):
            for shape in SHAPES:
                c = kernel_operands(shape, use_g, cuda)
                run_merge([c], s, cuda)
                check_bound(c, s, f"{shape} g={use_g} s={s} alone")
            cs = [kernel_operands(shape, use_g, cuda, seed=1) for shape in SHAPES]
            run_merge(cs, s, cuda)
            for c in cs:
                check_bound(c, s, f"{c.shape} g={use_g} s={s} five-record launch")


FWD_BAR = 3e-2  # tests/dora_ref.FWD_BAR, the bar tests/test_gpu_unet.py sets for the adapter path at these shapes


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def tiny_inputs(cfg, cuda):
    """tests/dora_ref.gpu_parity_case's inputs (B = 2), 16-bit valued."""
    from types import SimpleNamespace
    from pairwise_sample_optimization_amd import _lib
    elem = _lib.ELEM_DTYPE
    g = torch.Generator(device="cuda").manual_seed(0)
    B, h = 2, cfg.sample_size
    c = SimpleNamespace()
    c.sample = torch.randn(B, 4, h, h, device=cuda, generator=g).to(elem).float()
    c.t = torch.tensor([999.0, 499.0], device=cuda)
    c.enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(elem)
    c.text = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).to(elem)
    c.tid = torch.tensor([[8 * h, 8 * h, 0, 0, 8 * h, 8 * h]] * B, device=cuda, dtype=torch.float32)
    return c


def eps_nograd(unet, c):
    with torch.no_grad():
        return unet(c.sample, c.t, c.enc, added_cond_kwargs={"text_embeds": c.text, "time_ids": c.tid}).sample


def gpu_plain_case(r, cuda, b_std=0.1):
    """UNet case 1: tiny16 with a plain LoRA adapter of B ~ b_std N(0, 1) against the fp32 oracle on the same 16-bit
    valued weights: how far the adapter moves the oracle's eps, the adapter path's error and the fused path's."""
    from types import SimpleNamespace
    from oracle import sdxl_ref
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel(cfg).init_weights(0).to(cuda)
    unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    unet.lora.init_gaussian(seed=1, b_std=b_std)
    c = tiny_inputs(cfg, cuda)
    sd = sdxl_ref.sd_to(unet.state_dict(), cuda)
    lora = {k: v.float() for k, v in unet.lora.state_dict_peft().items()}
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)
    with torch.no_grad():
        e_base, e_lora = (sdxl_ref.unet_forward(sd, c.sample, c.t, c.enc.float(), c.text.float(), c.tid, lora=lo,
                                                cfg=ocfg) for lo in (None, lora))
    c.unet, c.moved = unet, rel(e_lora, e_base)
    c.adapter_err = rel(eps_nograd(unet, c), e_lora)
    unet.fuse_lora()
    assert unet.lora_fused is True
    c.fused_err = rel(eps_nograd(unet, c), e_lora)
    print(f"  tiny16 r={r} b_std={b_std}: oracle LoRA vs base {c.moved:.3e}; eps vs oracle: adapter path "
          f"{c.adapter_err:.3e}, fused {c.fused_err:.3e}", flush=True)
    return c
