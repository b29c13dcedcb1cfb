"""GPU cases of the fp16 library (libpso_amd_f16.so, PSO_LIB=f16): conversion semantics, one case per kernel family
that holds a matrix instruction or a 16-bit conversion, UNet / VAE parity against the fp32 oracle with torch's own fp16
as the yardstick, and fp16 training with dynamic loss scaling.

The module skips itself unless PSO_LIB=f16: the element type is per process, and the rest of the suite builds bf16
inputs for the bf16 library.  tests/test_f16_build.py::test_f16_library_on_gpu runs it in a child process.

Bars.  Single fp32-accumulate GEMMs on fp16-valued inputs: Frobenius relative error against the fp32 product <= 2^-10,
one fp16 ulp (half an ulp from the final rounding, plus a tie flipped by the summation order) -- derived, not measured.
Multi-stage kernels and whole networks: error against fp32 <= 1.5 x the error of the same torch computation run in
fp16 on the GPU (this project's convention for its torch-16-bit yardstick); both numbers are printed."""
import functools
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("PSO_LIB", "") != "f16",
                                 reason="fp16 library cases: run with PSO_LIB=f16 (tests/test_f16_build.py does)")]

ULP = 2.0 ** -10


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _h(*shape, g, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device="cuda", generator=g) * scale + shift).half()


def _yardstick(name, mine, torch16, ref32):
    e, y = _rel(mine, ref32), _rel(torch16, ref32)
    print(f"  {name}: f16 library {e:.3e}  torch fp16 {y:.3e}  (bar 1.5x = {1.5 * y:.3e})")
    assert torch.isfinite(mine.float()).all(), name
    assert e <= 1.5 * y, (name, e, y)


def _kernel(K):
    return K.lib().pso_last_kernel().decode()


def test_library_is_f16(cuda):
    import pairwise_sample_optimization_amd as pkg
    from pairwise_sample_optimization_amd import _lib
    assert _lib.lib().pso_elem_dtype() == _lib.PSO_F16 == 2 and pkg.compute_dtype() == torch.float16
    assert _lib.LIB_PATH.endswith("libpso_amd_f16.so")


# ----------------------------------------------------------------------------------------------------------------------
# 1. conversions, bit-exact against torch
# ----------------------------------------------------------------------------------------------------------------------
def test_casts_are_ieee_half_bit_exact(cuda):
    """f32 -> f16 is round-to-nearest-even with overflow to +-inf (never saturated), subnormals kept, NaN kept; the
    upcast is exact.  Vector path (16-B aligned, multiple of 8) and scalar tail both."""
    from pairwise_sample_optimization_amd import kernels as K
    special = [0.0, -0.0, 1.0, -1.0, 0.1, 1.0 / 3.0, 1000.7, 65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e6, -1e6,
               float("inf"), float("-inf"), float("nan"),
               1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2048.0 + 1.0, 2048.0 + 3.0,  # ties
               2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 6e-8,
               -5.9e-8, 1e-10]  # subnormals: ties at half the smallest subnormal, flush below
    g = _gen(1)
    x = torch.cat([torch.tensor(special, device=cuda),
                   torch.randn(4096, device=cuda, generator=g) * torch.exp(6 * torch.randn(4096, device=cuda, generator=g)),
                   torch.randn(3, device=cuda, generator=g)])  # length not a multiple of 8: scalar tail
    want = x.half()
    got = K.cast_f32_bf16(x)
    assert got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.isinf(got[11]) and torch.isinf(got[12]) and got[9].item() == 65504.0  # 65520 -> inf, 65519 -> 65504
    unaligned = K.cast_f32_bf16(x[1:])
    assert torch.equal(unaligned.view(torch.int16), want[1:].view(torch.int16))
    allbits = torch.arange(-32768, 32768, device=cuda, dtype=torch.int32).to(torch.int16).view(torch.float16)
    for src in (allbits, allbits[3:]):
        up = K.cast_bf16_f32(src)
        assert torch.equal(up.view(torch.int32), src.float().view(torch.int32))
    scaled = K.cast_f32_bf16(x, scale=0.5)
    assert torch.equal(scaled.view(torch.int16), (x * 0.5).half().view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------------
# 2. kernel families
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,form", [(200, 192, 72, "gemm_bf16_kernel<"), (6656, 2560, 128, "gemm8p_kernel<0,")])
def test_gemm_two_phase_and_eight_phase(cuda, M, N, K, form):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(M)
    a, w = _h(M, K, g=g), _h(N, K, g=g, scale=K ** -0.5)
    bias = _h(N, g=g)
    out = Kk.gemm(a, w, bias=bias)
    kn = _kernel(Kk)
    assert kn.startswith(form) and (form != "gemm8p_kernel<0," or ", 256, false>" in kn), kn
    assert out.dtype == torch.float16
    e = _rel(out, a.float() @ w.float().t() + bias.float())
    print(f"  gemm {M}x{N}x{K} [{kn}]: {e:.3e} (bar {ULP:.3e})")
    assert e <= ULP


def test_gemm_overflow_gives_inf_like_torch(cuda):
    """Integer-valued operands: every fp32 partial sum is exact in any order, so the output must equal the fp32
    product's .half() bit for bit -- +-inf where the sum is beyond 65520, no NaN, nothing saturated at 65504."""
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(7)
    M, N, K = 200, 192, 256
    a = torch.randint(-100, 101, (M, K), device=cuda, generator=g).half()
    w = torch.randint(-100, 101, (N, K), device=cuda, generator=g).half()
    ref = a.float() @ w.float().t()
    assert (ref.abs() > 65504).sum().item() > 100 and (ref.abs() < 60000).sum().item() > 100
    out = Kk.gemm(a, w)
    assert not torch.isnan(out).any()
    assert torch.equal(out.view(torch.int16), ref.half().view(torch.int16))
    assert torch.isinf(out).sum().item() == (ref.abs() >= 65520).sum().item() > 0
    acc = torch.zeros(M, N, device=cuda)
    Kk.gemm(a, w, out=acc, accumulate=True)  # the fp32 output keeps the sums
    assert torch.equal(acc, ref)


def test_gemm_split_k_workspace(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(3)
    M, N, K = 128, 128, 2048
    assert Kk.lib().pso_gemm_ws_bytes(M, N, K, 0) > 0
    a, w = _h(M, K, g=g), _h(N, K, g=g, scale=K ** -0.5)
    out = Kk.gemm(a, w)
    assert _kernel(Kk).startswith("gemm_bf16_kernel<128, 128")
    e = _rel(out, a.float() @ w.float().t())
    print(f"  split-K gemm: {e:.3e}")
    assert e <= ULP


def test_gemm_batched(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(4)
    a, w = _h(3, 100, 72, g=g), _h(3, 72, 72, g=g, scale=72 ** -0.5)
    out = Kk.gemm_batched(a, w)
    assert _kernel(Kk).startswith("gemm_bf16_kernel<64, 64")
    e = _rel(out, torch.bmm(a.float(), w.float().transpose(1, 2)))
    print(f"  batched gemm: {e:.3e}")
    assert out.dtype == torch.float16 and e <= ULP


def test_gemm_tn_and_rank_batch(cuda):
    """fp32 outputs (the LoRA / weight gradients): only the fp32 summation order separates them from torch."""
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(5)
    a, b = _h(77, 136, g=g), _h(77, 264, g=g)
    out = torch.zeros(136, 264, device=cuda)
    Kk.gemm_tn(a, b, out, alpha=0.5)
    assert _kernel(Kk) == "gemm_tn_kernel", _kernel(Kk)
    assert _rel(out, 0.5 * a.float().t() @ b.float()) < 1e-5
    x, u = _h(308, 256, g=g), _h(308, 32, g=g)
    q = Kk.TnRankQueue()
    o1, o2 = torch.zeros(256, 32, device=cuda), torch.zeros(32, 256, device=cuda)
    q.add(x, u, o1)
    q.add(u, x, o2)
    q.flush()
    assert _kernel(Kk).startswith("gemm_tn_rank_kernel<")
    ref = x.float().t() @ u.float()
    assert _rel(o1, ref) < 1e-5 and _rel(o2, ref.t()) < 1e-5


def test_gemm_skinny_grouped(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(6)
    M, C, G = 616, 320, 2
    a, w = _h(M, G * C, g=g), _h(32, G * C, g=g, scale=1 / 30)
    out = Kk.gemm_grouped_skinny(a, w, G)
    assert _kernel(Kk).startswith("gemm_skinny_nt_kernel<")
    ref = torch.cat([a[:, j * C:(j + 1) * C].float() @ w[:, j * C:(j + 1) * C].float().t() for j in range(G)], 1)
    e = _rel(out, ref)
    print(f"  grouped skinny: {e:.3e}")
    assert e <= ULP


def test_gemm_geglu_fwd_bwd(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(8)
    M, Fd, Kd = 300, 1280, 320
    x = _h(M, Kd, g=g)
    wp, bp = _h(2 * Fd, Kd, g=g, scale=Kd ** -0.5), _h(2 * Fd, g=g)
    idx = Kk.geglu_interleave_index(Fd, cuda)
    pre = torch.empty(M, 2 * Fd, device=cuda, dtype=torch.float16)
    out = Kk.gemm_geglu(x, wp[idx].contiguous(), bp[idx].contiguous(), out_pre=pre)
    assert _kernel(Kk).startswith("gemm8p_kernel<1,"), _kernel(Kk)
    hg32 = x.float() @ wp.float().t() + bp.float()
    hg16 = F.linear(x, wp, bp)
    _yardstick("geglu projection", out, hg16[:, :Fd] * F.gelu(hg16[:, Fd:]), hg32[:, :Fd] * F.gelu(hg32[:, Fd:]))
    assert _rel(pre, hg32[:, idx]) <= ULP
    # backward through ff.net.2: din = [dout * gelu(g) | dout * h * gelu'(g)] on the stored pre-activation
    dy, wo = _h(M, Kd, g=g), _h(Fd, Kd, g=g, scale=Kd ** -0.5)
    din = Kk.gemm_geglu_bwd(dy, wo, pre)
    assert _kernel(Kk).startswith("gemm_bf16_kernel<64, 64,"), _kernel(Kk)  # 24 tiles: the 2-phase GEGLU epilogue

    def ref(dtype):
        p = pre[:, torch.argsort(idx)].to(dtype).requires_grad_(True)  # natural [h | gate] order
        o = p[:, :Fd] * F.gelu(p[:, Fd:])
        (gp,) = torch.autograd.grad(o, p, F.linear(dy.to(dtype), wo.to(dtype)))
        return gp[:, idx]

    _yardstick("geglu backward", din, ref(torch.float16), ref(torch.float32))


def test_conv3x3(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(9)
    B, C, H, Co = 2, 64, 12, 96
    x = _h(B, H, H, C, g=g)
    w = _h(Co, 3, 3, C, g=g, scale=(9 * C) ** -0.5)
    b = _h(Co, g=g)
    out = Kk.conv2d(x, w, bias=b)
    assert _kernel(Kk).startswith("gemm_bf16_kernel<"), _kernel(Kk)
    run = lambda dt: F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt).permute(0, 3, 1, 2), b.to(dt), padding=1)
    _yardstick("conv 3x3", out.permute(0, 3, 1, 2), run(torch.float16), run(torch.float32))
    # the direct small-Cout form (the VAE's conv_out)
    x2 = _h(1, 16, 16, 64, g=g)
    w2 = _h(3, 3, 3, 64, g=g, scale=(9 * 64) ** -0.5)
    b2 = _h(3, g=g)
    out2 = Kk.conv2d(x2, w2, bias=b2)
    assert _kernel(Kk).startswith("conv3x3_smallc_kernel<3"), _kernel(Kk)
    run2 = lambda dt: F.conv2d(x2.to(dt).permute(0, 3, 1, 2), w2.to(dt).permute(0, 3, 1, 2), b2.to(dt), padding=1)
    _yardstick("conv 3x3 direct", out2.permute(0, 3, 1, 2), run2(torch.float16), run2(torch.float32))


def test_gemm_geglu_bwd_eight_phase(cuda):
    """The 8-phase 256 x 320 GEGLU backward (its MFMAs are inline asm): the smallest shape whose tiles make a whole
    round of 256 (64 x 4), at the shortest reduction the form takes."""
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(21)
    M, Fd, Kd = 16384, 1280, 64
    dy, wo = _h(M, Kd, g=g), _h(Fd, Kd, g=g, scale=Kd ** -0.5)
    pre = _h(M, 2 * Fd, g=g)  # interleaved [h 32 | gate 32] pre-activation
    din = Kk.gemm_geglu_bwd(dy, wo, pre)
    assert _kernel(Kk) == "gemm8p_kernel<2, true, false, false, 320, false>", _kernel(Kk)
    idx = Kk.geglu_interleave_index(Fd, cuda)

    def ref(dtype):
        p = pre[:, torch.argsort(idx)].to(dtype).requires_grad_(True)
        o = p[:, :Fd] * F.gelu(p[:, Fd:])
        (gp,) = torch.autograd.grad(o, p, F.linear(dy.to(dtype), wo.to(dtype)))
        return gp[:, idx]

    _yardstick("geglu backward 8-phase", din, ref(torch.float16), ref(torch.float32))


@pytest.mark.parametrize("B,H,Sq,Sk", [(2, 2, 256, 256), (2, 5, 300, 77)])
def test_attention_fwd_bwd(cuda, B, H, Sq, Sk):
    from pairwise_sample_optimization_amd import kernels as Kk
    C = H * 64
    g = _gen(Sq + Sk)
    q, k, v, do = _h(B, Sq, C, g=g), _h(B, Sk, C, g=g), _h(B, Sk, C, g=g), _h(B, Sq, C, g=g)
    o, lse = Kk.attention_fwd(q, k, v, H)
    dq, dk, dv = Kk.attention_bwd(q, k, v, o, lse, do, H)

    def run(dt):
        f = lambda t: t.to(dt).reshape(B, t.shape[1], H, 64).transpose(1, 2).detach().requires_grad_(True)
        qf, kf, vf = f(q), f(k), f(v)
        out = F.scaled_dot_product_attention(qf, kf, vf)
        grads = torch.autograd.grad(out, (qf, kf, vf), f(do).detach())
        back = lambda t: t.transpose(1, 2).reshape(B, -1, C)
        return [back(out)] + [back(t) for t in grads]

    r32, r16 = run(torch.float32), run(torch.float16)
    for name, mine, a16, a32 in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv), r16, r32):
        _yardstick(f"attention Sq={Sq} Sk={Sk} {name}", mine, a16, a32)
    f = lambda t: t.float().reshape(B, t.shape[1], H, 64).transpose(1, 2)
    assert (lse - torch.logsumexp(f(q) @ f(k).transpose(-1, -2) * 0.125, dim=-1)).abs().max().item() < 2e-3


@pytest.mark.parametrize("B,H,Sq,Sk", [(2, 5, 300, 77), (2, 2, 200, 191)])
def test_attention_strided_in_guarded_out(cuda, B, H, Sq, Sk):
    """The two ragged, query-split cases of tests/test_gpu_attention_layout.py on the fp16 library: strided inputs,
    outputs in guard-banded column slices, per-row error over all heads within 3 x the fp16 rounding model's."""
    import parity_util as P
    P.run_attention_case(cuda, B, H, Sq, Sk, True)


@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_fwd_bwd(cuda, silu):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(12)
    B, HW, C = 2, 100, 128
    x = _h(B, HW, C, g=g, scale=2.0, shift=0.5)
    gm, bt = _h(C, g=g, scale=0.1, shift=1.0), _h(C, g=g, scale=0.1)
    y, st = Kk.group_norm_fwd(x, gm, bt, 32, 1e-5, silu)
    dy = _h(B, HW, C, g=g)
    dx = Kk.group_norm_bwd(x, dy, st, gm, bt, silu)

    def run(dt):
        xr = x.to(dt).permute(0, 2, 1).detach().requires_grad_(True)
        o = F.group_norm(xr, 32, gm.to(dt), bt.to(dt), eps=1e-5)
        o = F.silu(o) if silu else o
        (gx,) = torch.autograd.grad(o, xr, dy.to(dt).permute(0, 2, 1))
        return o.permute(0, 2, 1), gx.permute(0, 2, 1)

    (y32, g32), (y16, g16) = run(torch.float32), run(torch.float16)
    _yardstick(f"group norm silu={silu} y", y, y16, y32)
    _yardstick(f"group norm silu={silu} dx", dx, g16, g32)


def test_layer_norm_fwd_bwd(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(13)
    M, C = 77, 320
    x = _h(M, C, g=g, shift=0.3)
    gm, bt = _h(C, g=g, scale=0.1, shift=1.0), _h(C, g=g, scale=0.1)
    y, st = Kk.layer_norm_fwd(x, gm, bt, 1e-5)
    dy = _h(M, C, g=g)
    dx = Kk.layer_norm_bwd(x, dy, st, gm)

    def run(dt):
        xr = x.to(dt).detach().requires_grad_(True)
        o = F.layer_norm(xr, (C,), gm.to(dt), bt.to(dt), 1e-5)
        (gx,) = torch.autograd.grad(o, xr, dy.to(dt))
        return o, gx

    (y32, g32), (y16, g16) = run(torch.float32), run(torch.float16)
    _yardstick("layer norm y", y, y16, y32)
    _yardstick("layer norm dx", dx, g16, g32)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("B,HW,C,G", [(2, 100, 320, 32), (1, 130, 1920, 32)])
def test_group_norm_localised(cuda, B, HW, C, G, silu):
    """Two GroupNorm cases of tests/test_gpu_norm_parity.py on the fp16 library (Cg = 10 across the 8-chunks; the
    480-thread block): saved statistics, per-chunk y / dx within 3 x the fp16 rounding model, dgamma / dbeta, guards."""
    import parity_util as P
    P.run_group_norm_case(cuda, B, HW, C, G, silu)


def test_layer_norm_localised(cuda):
    """The (7, 520) LayerNorm case of tests/test_gpu_norm_parity.py on the fp16 library: one chunk into MAXV = 2,
    strided inputs, guarded outputs."""
    import parity_util as P
    P.run_layer_norm_case(cuda, 7, 520)


@pytest.mark.parametrize("case", ["s1-straddle", "s2asym-vae"])
def test_conv_localised(cuda, case):
    """Two conv cases of tests/test_gpu_conv_guarded.py on the fp16 library (two images per 64-row tile with ragged
    M and N and the full epilogue; the VAE's asymmetric downsample): NaN-margined inputs, guarded output, the kernel
    name, every element within the bound derived for fp16."""
    import parity_util as P
    P.run_conv_case(cuda, case)


def test_geglu_elementwise_fwd_bwd(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(14)
    M, Fd = 77, 136
    h, dout = _h(M, 2 * Fd, g=g), _h(M, Fd, g=g)
    out, din = Kk.geglu_fwd(h), Kk.geglu_bwd(h, dout)

    def run(dt):
        p = h.to(dt).detach().requires_grad_(True)
        o = p[:, :Fd] * F.gelu(p[:, Fd:])
        (gp,) = torch.autograd.grad(o, p, dout.to(dt))
        return o, gp

    (o32, g32), (o16, g16) = run(torch.float32), run(torch.float16)
    _yardstick("geglu fwd", out, o16, o32)
    _yardstick("geglu bwd", din, g16, g32)


def test_adamw8bit_working_copy_is_master_half(cuda):
    from pairwise_sample_optimization_amd import kernels as Kk
    g = _gen(15)
    n = 2048 * 5 + 1003
    p = torch.randn(n, device=cuda, generator=g) * 0.02
    p[:4] = torch.tensor([70000.0, -70000.0, 3e-6, 65519.9], device=cuda)  # beyond the range, subnormal, near the edge
    st = Kk.Adam8State(n, cuda)
    wb = torch.full((n,), float("nan"), device=cuda, dtype=torch.float16)
    Kk.adamw8bit_step(p, torch.randn(n, device=cuda, generator=g) * 1e-2, st, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 1,
                      out_bf16=wb)
    assert torch.equal(wb.view(torch.int16), p.half().view(torch.int16))
    assert torch.isinf(wb[:2]).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3. UNet forward and LoRA-gradient parity; yardstick = the oracle under torch.autocast(float16)
# ----------------------------------------------------------------------------------------------------------------------
def _cfg(which):
    from pairwise_sample_optimization_amd.unet import UNetConfig
    return UNetConfig.tiny(16) if which == "tiny16" else UNetConfig.sdxl(32)


def _setup(cuda, cfg, B=2, r=8, seed=0):
    """tests/test_gpu_unet.py::_setup with the inputs rounded to fp16."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel
    unet = UNet2DConditionModel(cfg).init_weights(seed).to(cuda)
    unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    g = _gen(seed)
    h = cfg.sample_size
    sample = torch.randn(B, 4, h, h, device=cuda, generator=g).half().float()
    t = torch.tensor([999.0, 499.0][:B], device=cuda)
    enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).half()
    text = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).half()
    S = 8 * h
    tid = torch.tensor([[S, S, 0, 0, S, S]] * B, device=cuda, dtype=torch.float32)
    return unet, sample, t, enc, text, tid


def _tot(d, ref):
    return (sum(((d[k].float() - v) ** 2).sum().item() for k, v in ref.items()) /
            sum((v ** 2).sum().item() for v in ref.values())) ** 0.5


@functools.lru_cache(maxsize=None)
def _unet_parity(which):
    """One computation per config, shared by the tests below: the f16 library's eps and LoRA gradients, the fp32
    oracle's, and the oracle's under fp16 / bf16 autocast (same G, no loss scaling needed)."""
    from oracle import sdxl_ref
    cuda = torch.device("cuda:0")
    cfg = _cfg(which)
    unet, sample, t, enc, text, tid = _setup(cuda, cfg)
    assert unet.conv_in.weight.dtype == torch.float16
    G = torch.randn(sample.shape, device=cuda, generator=_gen(5))
    unet.lora.grad.zero_()
    out = unet(sample, t, enc, added_cond_kwargs={"text_embeds": text, "time_ids": tid}).sample
    (out * G).sum().backward()
    mine = {k: v.clone() for k, v in unet.lora.grad_dict_peft().items()}
    sd = sdxl_ref.sd_to(unet.state_dict(), cuda)
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)

    def oracle(dtype):
        leaf = {k: v.float().clone().requires_grad_(True) for k, v in unet.lora.state_dict_peft().items()}
        if dtype is None:
            o = sdxl_ref.unet_forward(sd, sample, t, enc.float(), text.float(), tid, lora=leaf, cfg=ocfg)
        else:
            with torch.autocast("cuda", dtype=dtype):
                o = sdxl_ref.unet_forward(sd, sample, t, enc.float(), text.float(), tid, lora=leaf, cfg=ocfg)
        (o.float() * G).sum().backward()
        return o.detach().float(), {k: v.grad for k, v in leaf.items()}

    e32, g32 = oracle(None)
    e16, g16 = oracle(torch.float16)
    eb, gb = oracle(torch.bfloat16)
    res = SimpleNamespace(out=out.detach(), mine=mine, e32=e32, g32=g32,
                          finite16=bool(torch.isfinite(e16).all() and all(torch.isfinite(v).all() for v in g16.values())),
                          eps=_rel(out, e32), eps16=_rel(e16, e32), epsb=_rel(eb, e32),
                          grad=_tot(mine, g32), grad16=_tot(g16, g32), gradb=_tot(gb, g32), n=len(g32))
    print(f"\n  {which}: eps  f16 library {res.eps:.3e}  autocast fp16 {res.eps16:.3e}  autocast bf16 {res.epsb:.3e}"
          f"\n  {which}: grads f16 library {res.grad:.3e}  autocast fp16 {res.grad16:.3e}  autocast bf16 {res.gradb:.3e}"
          f"  ({res.n} tensors, max |eps| {e32.abs().max().item():.2f})")
    return res


@pytest.mark.parametrize("which", ["tiny16", "sdxl32"])
def test_unet_forward_and_lora_grad_parity(cuda, which):
    r = _unet_parity(which)
    assert r.finite16, "precondition: the autocast-fp16 oracle is finite"
    assert set(r.mine) == set(r.g32) and r.n > 0  # no tensor is left out
    assert torch.isfinite(r.out).all() and all(torch.isfinite(v).all() for v in r.mine.values())
    assert r.eps <= 1.5 * r.eps16, (r.eps, r.eps16)
    assert r.grad <= 1.5 * r.grad16, (r.grad, r.grad16)
    # a library that still ran bf16 arithmetic could not be this close
    assert r.eps < 0.5 * r.epsb, (r.eps, r.epsb)
    assert r.grad < 0.5 * r.gradb, (r.grad, r.gradb)


def test_paired_pass_equals_separate_passes(cuda):
    """tests/test_gpu_unet.py::test_paired_pass_equals_separate_passes for tiny16 under f16, same bars."""
    from pairwise_sample_optimization_amd import kernels as K
    unet, sample, t, enc, text, tid = _setup(cuda, _cfg("tiny16"))
    x = K.nchw_to_nhwc(sample)
    assert x.dtype == torch.float16
    B = x.shape[0]
    st = unet.lora
    both, rt = unet.forward_nhwc(x, t, enc, text, tid, save=True, paired_ref=True)
    dout = torch.randn_like(both[:B].float()).half()
    st.grad.zero_()
    unet.backward_nhwc(dout, rt)
    g_pair = st.grad.clone()
    pol, rt1 = unet.forward_nhwc(x, t, enc, text, tid, save=True)
    st.grad.zero_()
    unet.backward_nhwc(dout, rt1)
    g_sep = st.grad.clone()
    unet.disable_adapters()
    with torch.no_grad():
        ref, _ = unet.forward_nhwc(x, t, enc, text, tid)
    unet.enable_adapters()
    e_pol, e_ref, e_g = _rel(both[:B], pol), _rel(both[B:], ref), _rel(g_pair, g_sep)
    print(f"  paired vs separate: policy {e_pol:.2e} reference {e_ref:.2e} lora grads {e_g:.2e}")
    assert both.shape[0] == 2 * B and both.dtype == torch.float16
    assert e_pol < 1e-2 and e_ref < 1e-2 and e_g < 3e-2
    assert (both[B:] - both[:B]).abs().max().item() > 0


# ----------------------------------------------------------------------------------------------------------------------
# 4. trainer: loss scaling, inf-skip, growth, graph re-capture, from_config
# ----------------------------------------------------------------------------------------------------------------------
def _trainer(cuda, loss_scale, use_8bit_adam=False, lr=1e-3):
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, lr=lr,
                    use_8bit_adam=use_8bit_adam, loss_scale=loss_scale)
    g = _gen(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).half()
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).half()
    tid = compute_time_ids(128, 0, cuda)
    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    sb = tr.shuffle(buf, generator=_gen(100))
    return unet, tr, sb


def _state(tr):
    ts = dict(tr.adam8.tensors()) if tr.adam8 is not None else {"exp_avg": tr.exp_avg, "exp_avg_sq": tr.exp_avg_sq}
    return {k: v.clone() for k, v in ts.items()}


def test_scaled_gradient_matches_unscaled(cuda):
    """(a) backward on loss * 1024, divided by 1024, against the S = 1 gradient: within the autocast-fp16 yardstick of
    the tiny16 parity case (the scale is a power of two: it moves fp16 roundings only at the range's edges).  The
    optimizer never runs here (auto_step off), so the AdamW kind does not enter."""
    grads = {}
    for S in (1.0, 1024.0):
        unet, tr, sb = _trainer(cuda, S)
        tr.auto_step = False
        unet.lora.grad.zero_()
        tr.train_epoch(sb)
        grads[S] = unet.lora.grad.clone()
        assert tr.loss_scale == S
    assert torch.isfinite(grads[1.0]).all() and torch.isfinite(grads[1024.0]).all() and grads[1.0].norm() > 0
    d = _rel(grads[1024.0] / 1024.0, grads[1.0])
    bar = _unet_parity("tiny16").grad16
    print(f"  unscaled S=1024 vs S=1: {d:.3e} (yardstick {bar:.3e})")
    assert d <= bar


@pytest.mark.parametrize("adam8", [False, True])
def test_overflow_skips_the_step_and_backs_off(cuda, adam8):
    """(b) an initial scale of 2^30 overflows the first backward (an arithmetic inf in fp16, not a fault): parameters,
    moments / 8-bit state and opt_step stay bit-unchanged, the gradient is zeroed, the scale halves; a later step at a
    workable scale updates the parameters."""
    unet, tr, sb = _trainer(cuda, 2.0 ** 30, use_8bit_adam=adam8)
    master0, work0, state0 = unet.lora.master.clone(), unet.lora.work.clone(), _state(tr)
    tr.train_epoch(sb)
    torch.cuda.synchronize()
    assert tr.opt_step == 0 and tr.scaler.scale == 2.0 ** 29 and tr.scaler.skipped == 1
    assert torch.equal(unet.lora.master, master0) and torch.equal(unet.lora.work, work0)
    for k, v in _state(tr).items():
        assert torch.equal(v, state0[k]), k
    assert unet.lora.grad.abs().max().item() == 0.0
    tr.scaler.scale = 1024.0
    tr.train_epoch(sb)
    torch.cuda.synchronize()
    assert tr.opt_step == 1 and tr.scaler.scale == 1024.0
    assert torch.isfinite(unet.lora.master).all() and not torch.equal(unet.lora.master, master0)
    assert unet.lora.grad.abs().max().item() == 0.0


@pytest.mark.parametrize("adam8", [False, True])
def test_scale_grows_after_clean_steps(cuda, adam8):
    """(c) growth interval 2: the scale doubles after two clean steps."""
    from pairwise_sample_optimization_amd.amp import LossScaler
    unet, tr, sb = _trainer(cuda, LossScaler(init_scale=256.0, growth_interval=2), use_8bit_adam=adam8)
    tr.train_epoch(sb)
    assert tr.scaler.scale == 256.0 and tr.opt_step == 1
    tr.train_epoch(sb)
    assert tr.scaler.scale == 512.0 and tr.opt_step == 2


@pytest.mark.parametrize("adam8", [False, True])
def test_graph_epoch_recaptures_on_scale_change(cuda, adam8):
    """(d) train_epoch_graph bakes the scale into the capture and re-captures when it changes: after a change the
    replayed gradient has the bits of the eager train_epoch at that scale."""
    u_g, tr_g, sb = _trainer(cuda, 256.0, use_8bit_adam=adam8)
    u_e, tr_e, _ = _trainer(cuda, 256.0, use_8bit_adam=adam8)
    tr_g.train_epoch_graph(sb)
    tr_e.train_epoch(sb)
    key0 = tr_g._graph_key
    assert tr_g._graph is not None and torch.equal(u_g.lora.master, u_e.lora.master)
    for tr in (tr_g, tr_e):
        tr.scaler.scale = 4096.0
    # the gradient of the epoch: stop the optimizer from consuming it
    seen = {}
    for name, tr, u in (("graph", tr_g, u_g), ("eager", tr_e, u_e)):
        tr.optimizer_step = lambda u=u, name=name: seen.__setitem__(name, u.lora.grad.clone())
    tr_g.train_epoch_graph(sb)
    tr_e.train_epoch(sb)
    torch.cuda.synchronize()
    assert tr_g._graph_key != key0 and ("loss_scale", 4096.0) in tr_g._graph_key
    assert seen["eager"].abs().max().item() > 0 and torch.isfinite(seen["eager"]).all()
    assert torch.equal(seen["graph"], seen["eager"])


def test_from_config_builds_fp16_training(cuda):
    """(e) both reference configs (mixed_precision = "fp16") build a trainer with scaling on; the DMD2 one replays the
    fp16 latent arithmetic; a bf16 or "no" config raises under this library."""
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.amp import LossScaler
    from pairwise_sample_optimization_amd.config import config_sdxl_dmd_dpo, config_sdxl_turbo_dpo
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.prepare()
    tt = PSOTrainer.from_config(unet, config_sdxl_turbo_dpo.get_config(), mode="turbo")
    td = PSOTrainer.from_config(unet, config_sdxl_dmd_dpo.get_config(), mode="dmd")
    for tr in (tt, td):
        assert isinstance(tr.scaler, LossScaler) and tr.loss_scale == 65536.0 and tr.scaler.growth_interval == 2000
    assert td.mode == _lib.MODE_DMD_F16 and td.latent_dtype == torch.float16 and tt.mode == _lib.MODE_TURBO
    cfg = config_sdxl_turbo_dpo.get_config()
    cfg.mixed_precision = "bf16"
    with pytest.raises(ValueError, match="fp16"):
        PSOTrainer.from_config(unet, cfg, mode="turbo")
    cfg.mixed_precision = "no"
    with pytest.raises(ValueError, match="fp16"):
        PSOTrainer.from_config(unet, cfg, mode="turbo")


@pytest.mark.parametrize("name", ["dmd_replay_bf16_P2_h16_t499.npz", "dmd_replay_fp16_P2_h16_t999.npz"])
def test_dmd_latent_dtype_replay_is_independent_of_the_element_type(cuda, name):
    """The DMD2 replay modes round to the LATENT dtype the caller names (PSO_MODE_DMD_BF16 / _F16), whatever the
    library's element type: the reference's executed bf16 and fp16 steps (tests/golden, the bars of
    tests/test_gpu_reference_fixtures.py) hold on the f16 library too -- prev bit-exact, log-probs within one
    latent-dtype ulp, loss rtol 1e-5.  A bf16 mode that rounded through the element type would give fp16 bits."""
    import numpy as np
    from pairwise_sample_optimization_amd import kernels as K, pso_core
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    lat = torch.float16 if str(d["latent"]) == "fp16" else torch.bfloat16
    mode = pso_core.dmd_mode(lat)
    ulp = 2.0 ** -10 if lat == torch.float16 else 2.0 ** -7
    P = d["x0"].shape[0]
    coef = pso_core.dmd_coef(torch.from_numpy(d["alphas_cumprod"]), torch.from_numpy(d["t"]),
                             torch.from_numpy(d["t_prev"]), latent_dtype=lat).to(cuda)
    T = lambda k: torch.from_numpy(d[k]).to(cuda)
    for k in range(2):
        prev, lp = K.step_logprob(mode, T(f"x{k}"), T(f"eps_ref{k}"), coef, noise=T(f"noise{k}"), noise_shared=P > 1)
        np.testing.assert_array_equal(prev.cpu().numpy(), d[f"prev{k}"])
        assert torch.equal(prev, prev.to(lat).float())  # latent-dtype valued
        np.testing.assert_allclose(lp.cpu().numpy(), d[f"lp_sample{k}"], rtol=ulp)
    inter = lambda a, b: torch.stack([T(a), T(b)], 1).reshape((2 * P,) + d["x0"].shape[1:]).contiguous()
    x, xp = inter("x0", "x1"), inter("prev0", "prev1")
    ep, er = inter("eps_pol0", "eps_pol1"), inter("eps_ref0", "eps_ref1")
    coef2 = torch.stack([coef, coef], 1).reshape(2 * P, -1).contiguous()
    ws = K.pair_loss_ws(P, x[0].numel(), cuda)
    loss, lp = K.pair_loss_fwd(mode, x, xp, ep, er, coef2, T("pref"), float(d["beta"]), float(d["clip_eps"]), ws)
    lp = lp.cpu().numpy().reshape(P, 2, 2)
    for k in range(2):
        np.testing.assert_allclose(lp[:, k, 0], d[f"lp_pol{k}"], rtol=ulp)
        np.testing.assert_allclose(lp[:, k, 1], d[f"lp_ref{k}"], rtol=ulp)
    np.testing.assert_allclose(loss.item(), d["loss"], rtol=1e-5)


# ----------------------------------------------------------------------------------------------------------------------
# 5. VAE decode; 6. guards
# ----------------------------------------------------------------------------------------------------------------------
def test_vae_decode_parity(cuda):
    from oracle import sdxl_ref
    from pairwise_sample_optimization_amd.vae import AutoencoderKL, VAEConfig
    with torch.device(cuda):
        vae = AutoencoderKL(VAEConfig.tiny())
    vae.init_weights(0)
    h = 16
    z = torch.randn(2, 4, h, h, device=cuda, generator=_gen(0)).half().float()
    zin = (z / vae.config.scaling_factor).half().float()
    img = vae.decode(z / vae.config.scaling_factor, return_dict=False)[0]
    sd = sdxl_ref.sd_to(vae.state_dict(), cuda)
    ref = sdxl_ref.vae_decode(sd, zin)
    with torch.autocast("cuda", dtype=torch.float16):
        ref16 = sdxl_ref.vae_decode(sd, zin)
    assert img.shape == (2, 3, 8 * h, 8 * h) and torch.isfinite(ref16).all()
    _yardstick("vae decode tiny h=16", img, ref16.float(), ref)


def test_paths_not_verified_in_fp16_raise(cuda):
    from pairwise_sample_optimization_amd import _lib, clip
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        unet.enable_full_grads()
    assert unet.full is None
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        unet.enable_fp8_forward()
    assert not getattr(unet, "fp8", False)
    unet.enable_fp8_forward(False)  # switching it off is always allowed
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        clip.CLIPTextModel(clip.CLIPTextConfig())
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        clip.CLIPVisionTransformer(clip.CLIPVisionConfig())
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    with pytest.raises(_lib.PsoLibError, match="f16 library"):  # code 2 means uint8 to that entry, not fp16
        K.clip_preprocess(torch.zeros(1, 32, 32, 3, device=cuda, dtype=torch.float16), 28, 14, 592, (0.5,) * 3, (0.5,) * 3)
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        DreamBoothPSOTrainer(unet, None)
    with pytest.raises(_lib.PsoLibError, match="PSO_LIB"):
        _lib.dtype_code(torch.zeros(2, device=cuda, dtype=torch.bfloat16))
    # the library itself refuses the other 16-bit code and names the library to load
    from pairwise_sample_optimization_amd.kernels import ptr, stream_ptr
    x = torch.zeros(2, 4, 8, device=cuda)
    y = torch.zeros(2, 8, 4, device=cuda, dtype=torch.float16)
    rc = _lib.lib().pso_nchw_to_nhwc(2, 4, 4, 8, ptr(x), _lib.PSO_BF16, 1.0, ptr(y), stream_ptr())
    assert rc == 1 and b"libpso_amd.so" in _lib.lib().pso_last_error()
