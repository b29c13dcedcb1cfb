"""Shared pieces of the localised-error parity tests (a plain module: no fixtures, no hooks).

Why it exists: a whole-tensor Frobenius ratio ||a - b|| / ||b|| cannot see an error confined to one query row of one
head, one 4-element store chunk or the last key of a ragged tile -- the errors a tiled kernel makes -- and a fresh
contiguous output tensor cannot show a store that lands beside the slice it was meant for.  So:

  rowwise_rel      worst per-(row, 64-wide group) relative error, with its index
  guarded          output views inside a buffer whose every other element must keep its fill pattern, bit for bit
  attention_model  the attention kernels' documented roundings restated in plain torch (sets the per-row bound)
  attention_fp64   the reference
  geglu_* / gemm_* cases, fp64 references and derived element-wise bounds of the GEMM epilogue tests

Everything here runs on whatever device its inputs are on; tests/test_parity_util.py exercises it without a GPU.
"""
import math

import torch

_TINY = 1e-300


# ----------------------------------------------------------------------------------------------------------------------
# per-row metric
# ----------------------------------------------------------------------------------------------------------------------
class RowErr(float):
    """The worst per-group-row relative error (a float) with .index, the position of that group-row in
    got.shape[:-1] + (got.shape[-1] // width,): (batch, row, head) for a [B, S, H*64] attention tensor."""

    def __new__(cls, value, index):
        self = super().__new__(cls, value)
        self.index = index
        return self

    def __repr__(self):
        return f"{float(self):.3e} at {self.index}"

    __str__ = __repr__


def rowwise_rel(got, ref, width):
    """max over group-rows of ||got - ref||_2 / ||ref||_2 in fp64, the last dimension taken in groups of `width`
    (64 = one attention head).  A NaN anywhere in `got` comes back as NaN, which fails every `<` assertion."""
    assert got.shape == ref.shape and got.shape[-1] % width == 0, (got.shape, ref.shape, width)
    g = got.detach().to(torch.float64).reshape(-1, width)
    r = ref.detach().to(torch.float64).reshape(-1, width)
    err = (g - r).norm(dim=1) / r.norm(dim=1).clamp_min(_TINY)
    bad = torch.isnan(err)
    i = int(bad.nonzero()[0]) if bool(bad.any()) else int(err.argmax())
    lead = tuple(got.shape[:-1]) + (got.shape[-1] // width,)
    idx = []
    for n in reversed(lead):
        idx.append(i % n)
        i //= n
    return RowErr(err.max().item() if not bool(bad.any()) else float("nan"), tuple(reversed(idx)))


def frob_rel(got, ref):
    """The whole-tensor ratio the older parity tests use, in fp64 (kept to show what it cannot see)."""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64)
    return ((g - r).norm() / r.norm().clamp_min(_TINY)).item()


# ----------------------------------------------------------------------------------------------------------------------
# guard bands
# ----------------------------------------------------------------------------------------------------------------------
# NaNs with a payload, for bf16 / fp16 (0x7FA5) and fp32 (0x7FA5A5A5): not zero, not the canonical quiet NaN a kernel or
# torch would produce (0x7FC0 / 0x7E00 / 0x7FC00000), so a stray store of any computed value changes the bits, and a
# stray load of a guard element poisons what is computed from it.
FILL_BITS = {2: 0x7FA5, 4: 0x7FA5A5A5}
_IVIEW = {2: torch.int16, 4: torch.int32}


def guarded(shape_rows, widths, gap=8, guard_rows=64, dtype=None, device=None):
    """One [shape_rows + guard_rows, ld] buffer whose rows are laid out [gap | w0 | gap | w1 | gap | ... | gap] (the
    last gap padded so that ld is a multiple of 8 elements), every element holding one fixed NaN-payload bit pattern.
    Returns (views, check): the [shape_rows, w_i] column-slice views (16-byte aligned: gap = 8 elements of 2 bytes)
    and a closure asserting that every element outside the views still holds the fill, compared as integers (NaN !=
    NaN); on a mismatch it names the first touched (row, column) of the buffer."""
    if dtype is None:
        from pairwise_sample_optimization_amd import kernels as K
        dtype = K.ELEM
    size = torch.empty((), dtype=dtype).element_size()
    fill, ivt = FILL_BITS[size], _IVIEW[size]
    ld = gap + sum(w + gap for w in widths)
    ld = -(-ld // 8) * 8
    rows = shape_rows + guard_rows
    buf = torch.empty((rows, ld), dtype=dtype, device=device)
    ibuf = buf.view(ivt)
    ibuf.fill_(fill)
    views, spans, c = [], [], gap
    for w in widths:
        views.append(buf[:shape_rows, c:c + w])
        spans.append((c, c + w))
        c += w + gap

    def check(what="guard band"):
        touched = ibuf != fill
        for c0, c1 in spans:
            touched[:shape_rows, c0:c1] = False
        if bool(touched.any()):
            r, col = (int(t) for t in touched.nonzero()[0])
            where = "a guard row" if r >= shape_rows else "a gap column"
            raise AssertionError(f"{what}: {int(touched.sum())} element(s) outside the output views were written; "
                                 f"first at (row {r}, column {col}) of the [{rows}, {ld}] buffer ({where}; views are "
                                 f"rows 0..{shape_rows - 1}, columns {spans}), bits {int(ibuf[r, col]) & (2 ** (8 * size) - 1):#x}")

    return views, check


# ----------------------------------------------------------------------------------------------------------------------
# attention: inputs the way unet.py passes them, the rounding model, the fp64 reference
# ----------------------------------------------------------------------------------------------------------------------
# (B, H, Sq, Sk) -> does the backward split the queries (pso_attention_bwd_ws_bytes carries split partials)?
# Forward tile: 256 queries per workgroup when cdiv(Sq, 256) * H * B >= 1024 and Sk > 128, else 128 (pso_attention_fwd).
# Backward: Sk <= 96 the one-pass x kernel; 96 < Sk <= 256 dQ + dK/dV kernels with query splits when there are few key
# blocks; Sk > 256 dQ + dK/dV, never split (cross_qsplit in attention.hip).
ATTN_CASES = {
    # fwd-128 / x kernel, one query tile: Sq < 64, Sk no multiple of 16 or 32
    (1, 1, 1, 5): False,
    (2, 2, 50, 77): False,
    # x kernel, split (512 / (H * B) = 51 -> 5 query tiles), ragged last query tile
    (2, 5, 300, 77): True,
    # x kernel at its key limit, one row into the second query tile (two tiles -> two splits)
    (1, 3, 65, 96): True,
    # x kernel, head offsets up to 19
    (2, 20, 130, 77): True,
    # mid path, one query tile -> no split
    (1, 2, 60, 130): False,
    # mid path, split: reduce_splits_kernel writes through lddk / lddv; ragged key tile
    (2, 2, 200, 191): True,
    # self-attention from a fused qkv, ragged and exact tiles (mid path, split)
    (1, 2, 100, 100): True,
    (2, 2, 256, 256): True,
    # long keys: Sk > 256, never split, ragged 128-key block
    (1, 2, 130, 300): False,
}
# cdiv(300, 256) * 8 * 64 = 1024 and Sk = 130 > 128: attn_fwd2_kernel<4> by the product dispatch, ragged second block
ATTN_FWD256_CASE = (64, 8, 300, 130)
ATTN_RAGGED_CASES = [(2, 5, 300, 77), (2, 2, 200, 191)]


def attention_inputs(B, H, Sq, Sk, dtype, device, seed=None):
    """q, k, v, do as unet.py hands them over: column slices of one [B, S, 3C] tensor when Sq == Sk, else q from
    [B, Sq, C] and k, v the two halves of a [B, Sk, 2C] tensor; do contiguous.  Drawn on the CPU from a fixed seed, so
    the CPU self-test and the GPU tests see the same numbers."""
    C = H * 64
    g = torch.Generator().manual_seed(1000 * Sq + Sk + H if seed is None else seed)
    if Sq == Sk:
        qkv = torch.randn(B, Sq, 3 * C, generator=g).to(dtype).to(device)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        q = torch.randn(B, Sq, C, generator=g).to(dtype).to(device)
        kv = torch.randn(B, Sk, 2 * C, generator=g).to(dtype).to(device)
        k, v = kv[..., :C], kv[..., C:]
    do = torch.randn(B, Sq, C, generator=g).to(dtype).to(device)
    return q, k, v, do


def _heads(t, H, dt):
    B, S, _ = t.shape
    return t.reshape(B, S, H, 64).transpose(1, 2).to(dt)  # [B, H, S, 64]


def _merge(t):
    B, H, S, _ = t.shape
    return t.transpose(1, 2).reshape(B, S, H * 64)


def attention_model(q, k, v, do, H, scale):
    """The kernels' documented roundings in plain torch (attention.hip's header and kernel comments): fp32 scores from
    the 16-bit inputs, fp32 softmax, P rounded to the element type before P . V, O rounded to the element type;
    delta = rowsum(dO * O) from the rounded O; P and dS rounded to the element type before the dQ / dK / dV products;
    every accumulation in fp32; outputs rounded to the element type.  Returns (o, lse, dq, dk, dv); do=None: (o, lse)."""
    et = q.dtype
    qf, kf, vf = (_heads(t, H, torch.float32) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m).to(et).float()
    # the row sum is taken on the matrix cores from the rounded P (attention.hip: lsum = mfma16x16x32(ones, pf, lsum))
    l = p.sum(-1, keepdim=True)
    o = ((p @ vf) / l).to(et)
    lse = (m + torch.log(l)).squeeze(-1)
    if do is None:
        return _merge(o), lse
    dof = _heads(do, H, torch.float32)
    pn = torch.exp(s - lse.unsqueeze(-1))            # the backward recomputes P from Q, K and the saved LSE
    delta = (dof * o.float()).sum(-1, keepdim=True)
    ds = (pn * (dof @ vf.transpose(-1, -2) - delta)).to(et).float()
    pn = pn.to(et).float()
    dv = (pn.transpose(-1, -2) @ dof).to(et)
    dk = ((ds.transpose(-1, -2) @ qf) * scale).to(et)
    dq = ((ds @ kf) * scale).to(et)
    return _merge(o), lse, _merge(dq), _merge(dk), _merge(dv)


def attention_fp64(q, k, v, do, H, scale):
    """The same mathematics in fp64 from the same 16-bit inputs, nothing rounded: (o, lse, dq, dk, dv), all fp64;
    do=None: (o, lse)."""
    qf, kf, vf = (_heads(t, H, torch.float64) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ vf
    if do is None:
        return _merge(o), lse
    dof = _heads(do, H, torch.float64)
    delta = (dof * o).sum(-1, keepdim=True)
    ds = p * (dof @ vf.transpose(-1, -2) - delta)
    return _merge(o), lse, _merge(ds @ kf * scale), _merge(ds.transpose(-1, -2) @ qf * scale), \
        _merge(p.transpose(-1, -2) @ dof)


# Why 3: the kernel's accumulation order, its exp2 path with the deferred rescale and its in-kernel -delta are each a
# further rounding of the size of the modelled ones (2 would cover them if they doubled the error); the third unit is
# slack for the extreme-value statistic of a maximum over a few thousand rows.  A local fault (one wrong 4-element chunk
# of a 64-wide row) moves its row by sqrt(4 / 64) = 0.25, fifty times the model's worst row.
ROW_BOUND_FACTOR = 3.0


def attention_row_bounds(model, ref64):
    """bound = 3 x (worst per-row error of attention_model against attention_fp64), per tensor o / dq / dk / dv: it
    comes from the reference side alone, never from a kernel's output."""
    names = ("o", "dq", "dk", "dv") if len(model) == 5 else ("o",)
    pick = {"o": 0, "dq": 2, "dk": 3, "dv": 4}
    return {n: rowwise_rel(model[pick[n]], ref64[pick[n]], 64) for n in names}


def qsplit_from_ws_bytes(ws_bytes, B, H, Sq, Sk):
    """The backward's query split, read off pso_attention_bwd_ws_bytes: two 256-byte-rounded [B][H][Sq] fp32 blocks
    (-delta and the LSE in log2 units), then -- only when the queries are split -- 2 * qsplit fp32 [B][Sk][H*64]
    partial slices."""
    d = -(-(B * H * Sq * 4) // 256) * 256
    acc = ws_bytes - 2 * d
    one = 2 * B * Sk * H * 64 * 4
    assert acc >= 0 and acc % one == 0, (ws_bytes, d, one)
    return acc // one if acc else 1


ATTN_SCALE = 64 ** -0.5


def run_attention_case(cuda, B, H, Sq, Sk, expect_split, backward=True):
    """One case of tests/test_gpu_attention_layout.py (and of the fp16 library's in tests/test_gpu_f16.py): strided
    inputs, guarded outputs, the five assertions.  expect_split: whether the backward splits the queries."""
    from pairwise_sample_optimization_amd import kernels as K
    C = H * 64
    q, k, v, do = attention_inputs(B, H, Sq, Sk, K.ELEM, cuda)
    assert not q.is_contiguous() or Sq != Sk  # the fused-qkv slices are row-strided
    assert not k.is_contiguous() and not v.is_contiguous()
    if not backward:
        do = None
    ref = attention_fp64(q, k, v, do, H, ATTN_SCALE)
    model = attention_model(q, k, v, do, H, ATTN_SCALE)
    worst_model = attention_row_bounds(model, ref)

    (o2,), check_o = guarded(B * Sq, [C], device=cuda)
    o = o2.view(B, Sq, C)
    got_o, lse = K.attention_fwd(q, k, v, H, out=o)
    assert got_o.data_ptr() == o.data_ptr()
    got = {"o": o}
    checks = [("forward out", check_o)]
    if backward:
        if Sq == Sk:  # d3-style: dq | dk | dv slices of one buffer
            (dq2, dk2, dv2), check_d = guarded(B * Sq, [C, C, C], device=cuda)
            checks.append(("backward dq|dk|dv", check_d))
        else:         # dq alone, dk | dv slices of a second buffer
            (dq2,), check_dq = guarded(B * Sq, [C], device=cuda)
            (dk2, dv2), check_dkv = guarded(B * Sk, [C, C], device=cuda)
            checks += [("backward dq", check_dq), ("backward dk|dv", check_dkv)]
        dq, dk, dv = dq2.view(B, Sq, C), dk2.view(B, Sk, C), dv2.view(B, Sk, C)
        assert dk.stride(0) == Sk * dk.stride(1) and dv.stride(0) == Sk * dv.stride(1)  # the split path needs it
        qsplit = qsplit_from_ws_bytes(K.lib().pso_attention_bwd_ws_bytes(B, H, Sq, Sk), B, H, Sq, Sk)
        assert (qsplit > 1) == expect_split, f"query split {qsplit}: the case no longer reaches its regime"
        K.attention_bwd(q, k, v, o, lse, do, H, dq=dq, dk=dk, dv=dv)
        got.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    for what, chk in checks:   # 1. nothing outside the slices changed, the 64 guard rows included
        chk(f"{(B, H, Sq, Sk)} {what}")
    pick = {"o": 0, "dq": 2, "dk": 3, "dv": 4}
    line = []
    for name, x in got.items():
        e = rowwise_rel(x, ref[pick[name]], 64)
        line.append(f"{name} kernel {e} model {worst_model[name]}")
    print(f"\n[rows {K.ELEM} {(B, H, Sq, Sk)}] " + "; ".join(line)
          + f"; lse {(lse.double() - ref[1]).abs().max().item():.2e}", flush=True)
    for name, x in got.items():
        assert torch.isfinite(x.float()).all(), name                    # 3.
        e = rowwise_rel(x, ref[pick[name]], 64)                         # 2. per (batch, row, head), all heads
        bound = ROW_BOUND_FACTOR * worst_model[name]
        assert e < bound, (f"{(B, H, Sq, Sk)} {name}: worst row {e} (batch, row, head), bound {bound:.3e} = 3 x model "
                           f"{worst_model[name]}")
    assert torch.isfinite(lse).all()
    assert (lse.double() - ref[1]).abs().max().item() < 2e-3              # 4.


# ----------------------------------------------------------------------------------------------------------------------
# GEGLU epilogues: element-wise bounds derived from the number formats
# ----------------------------------------------------------------------------------------------------------------------
GEGLU_CASES = [(300, 1280, 320, 100),   # ragged M, pre_rows in the middle of a tile
               (257, 640, 128, 0),      # one row into a second 256-row tile
               (64, 320, 64, 64),       # smaller than any tile; 2 * Fd = 640 is no multiple of 256: the forward
                                        # refuses it (an argument error), the backward takes it
               (64, 384, 64, 64)]       # smaller than any tile, and a width the forward takes
U16 = 2.0 ** -8    # one bf16 rounding: 8 significant bits, unit roundoff 2^-8
U32 = 2.0 ** -23   # one fp32 rounding (unit roundoff 2^-24), doubled


def _interleave_index(Fd, device):
    g = torch.arange(Fd // 32, device=device).view(-1, 1)
    j = torch.arange(32, device=device).view(1, -1)
    return torch.cat([g * 32 + j, Fd + g * 32 + j], 1).reshape(-1)


def _gelu_parts(g):
    cdf = 0.5 * torch.erfc(-g / math.sqrt(2.0))  # Phi(g) without the 1 + erf cancellation, as gelu_erf_parts forms it
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    return g * cdf, cdf + g * pdf   # gelu(g), gelu'(g)


def geglu_inputs(M, Fd, K, device):
    """bf16 operands of one GEGLU case in diffusers' natural [h rows; gate rows] order, drawn on the CPU."""
    g = torch.Generator().manual_seed(M + Fd + K)
    bf = lambda t: t.bfloat16().to(device)
    return dict(x=bf(torch.randn(M, K, generator=g)), wp=bf(torch.randn(2 * Fd, K, generator=g) / K ** 0.5),
                bp=bf(torch.randn(2 * Fd, generator=g)), dy=bf(torch.randn(M, K, generator=g)),
                wo=bf(torch.randn(Fd, K, generator=g) / K ** 0.5))


def geglu_reference(inp, Fd):
    """fp64 references and element-wise bounds for gemm_geglu (out, interleaved out_pre) and gemm_geglu_bwd.

    The pre-activation may differ from fp64 by d = 2^-8 |pre| + (K + 8) 2^-23 (|x| |w|^T + |b|): one bf16 rounding and
    an fp32 accumulation in any order (doubled).  out = h * gelu(g) moves to first order by |gelu(g)| d_h +
    |h gelu'(g)| d_g, plus 2^-8 |out| for its own rounding.  The backward's two halves dout gelu(g) and
    dout h gelu'(g) are built the same way, from d_h, d_g and dout's own d_dout = 2^-8 |dout| + (K + 8) 2^-23 |dy| |wo|^T.  Outputs are in the kernels' interleaved [h 32 | gate 32] column order where the
    kernels interleave."""
    x, wp, bp, dy, wo = (inp[n].double() for n in ("x", "wp", "bp", "dy", "wo"))
    K = x.shape[1]
    idx = _interleave_index(Fd, x.device)
    pre = x @ wp.t() + bp
    d = U16 * pre.abs() + (K + 8) * U32 * (x.abs() @ wp.abs().t() + bp.abs())
    h, g = pre[:, :Fd], pre[:, Fd:]
    gelu, dgelu = _gelu_parts(g)
    out = h * gelu
    out_bound = gelu.abs() * d[:, :Fd] + (h * dgelu).abs() * d[:, Fd:] + U16 * out.abs()
    # The backward is handed the bf16 rounding of the reference's pre-activation -- what the forward stores, to within
    # d -- and is compared with the fp64 result at the UNROUNDED h, g: so d_h, d_g go through its epilogue like the
    # forward's, and dout = dy wo^T brings its own d.  gelu''(g) = phi(g) (2 - g^2).
    pre_in = pre.bfloat16()
    dout = dy @ wo.t()
    dd = U16 * dout.abs() + (K + 8) * U32 * (dy.abs() @ wo.abs().t())
    ddgelu = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi) * (2 - g * g)
    din = torch.cat([dout * gelu, dout * h * dgelu], 1)
    din_bound = torch.cat([gelu.abs() * dd + (dout * dgelu).abs() * d[:, Fd:],
                           (h * dgelu).abs() * dd + (dout * dgelu).abs() * d[:, :Fd]
                           + (dout * h * ddgelu).abs() * d[:, Fd:]], 1) + U16 * din.abs()
    return dict(idx=idx, pre=pre[:, idx], pre_bound=d[:, idx], out=out, out_bound=out_bound,
                pre_in=pre_in[:, idx].contiguous(), din=din[:, idx], din_bound=din_bound[:, idx])


def geglu_restatement(inp, Fd, pre_in):
    """What the kernels are documented to compute, in torch: fp32 matmul, pre-activation rounded to bf16, epilogue in
    fp32, output rounded to bf16.  Returns (out, out_pre interleaved, din interleaved)."""
    x, wp, bp, dy, wo = (inp[n].float() for n in ("x", "wp", "bp", "dy", "wo"))
    idx = _interleave_index(Fd, x.device)
    pre = (x @ wp.t() + bp).bfloat16()
    h, g = pre[:, :Fd].float(), pre[:, Fd:].float()
    out = (h * _gelu_parts(g)[0]).bfloat16()
    pi = torch.empty_like(pre_in)
    pi[:, idx] = pre_in                      # back to the natural order
    hb, gb = pi[:, :Fd].float(), pi[:, Fd:].float()
    gelu_b, dgelu_b = _gelu_parts(gb)
    dout = (dy @ wo.t()).bfloat16().float()
    din = torch.cat([dout * gelu_b, dout * hb * dgelu_b], 1).bfloat16()
    return out, pre[:, idx], din[:, idx]


def violations(got, ref, bound):
    """(count, message): elements with |got - ref| > bound (NaN counts), and where the worst one is."""
    err = (got.detach().double() - ref).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if not n:
        return 0, ""
    ratio = torch.where(bad, err / bound.clamp_min(_TINY), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    r, c = i // got.shape[1], i % got.shape[1]
    return n, (f"{n} of {got.numel()} elements outside the bound; worst at (row {r}, column {c}): got "
               f"{float(got[r, c]):.6g}, ref {float(ref[r, c]):.6g}, bound {float(bound[r, c]):.3g}")


# ----------------------------------------------------------------------------------------------------------------------
# plain gemm: one small ragged case per dispatch family
# ----------------------------------------------------------------------------------------------------------------------
# id -> (variant, M, N, K, K2, tail_group_n, tail_rows, mode, kernel-name prefix)
#   variant: the pso_gemm_set_variant knob that pins the family at this size (0 = the product dispatch)
#   mode:    "bias" bf16 out with alpha and bias; "resid" the same plus a bf16 residual; "acc" fp32 out, accumulate
#            (the accumulator's previous contents stand in the bound's |resid| place); "plain" bf16 out, alpha only
GEMM_CASES = {
    "2phase-bias": (0, 300, 256, 128, 0, 0, 0, "bias", "gemm_bf16_kernel<64, 64,"),
    "2phase-resid": (0, 300, 256, 128, 0, 0, 0, "resid", "gemm_bf16_kernel<64, 64,"),
    "2phase-acc": (0, 300, 256, 128, 0, 0, 0, "acc", "gemm_bf16_kernel<64, 64,"),
    "2phase-tail-grouped-rows": (0, 300, 256, 128, 32, 128, 100, "resid", "gemm_bf16_kernel<64, 64,"),
    "2phase-tail-acc": (0, 300, 256, 128, 32, 0, 0, "acc", "gemm_bf16_kernel<64, 64,"),
    "8phase-256x256": (30, 300, 256, 128, 0, 0, 0, "bias", "gemm8p_kernel<0, true, false, false, 256,"),
    "8phase-256x256-resid": (30, 1000, 768, 640, 0, 0, 0, "resid", "gemm8p_kernel<0, true, false, false, 256,"),
    "8phase-256x256-tail": (30, 300, 512, 192, 32, 256, 100, "resid", "gemm8p_kernel<0, true, false, false, 256,"),
    "8phase-256x160": (38, 300, 320, 192, 0, 0, 0, "resid", "gemm8p_kernel<0, true, false, false, 160,"),
    "8phase-256x160-tail": (38, 257, 640, 64, 96, 320, 100, "bias", "gemm8p_kernel<0, true, false, false, 160,"),
    "8phase-256x320": (39, 300, 320, 192, 0, 0, 0, "resid", "gemm8p_kernel<0, true, false, false, 320,"),
    "8phase-256x320-tail": (39, 257, 640, 192, 32, 320, 100, "bias", "gemm8p_kernel<0, true, false, false, 320,"),
    "skinny": (0, 300, 100, 136, 0, 0, 0, "plain", "gemm_skinny_nt_kernel<"),
    "skinny-acc": (0, 300, 100, 136, 0, 0, 0, "acc", "gemm_skinny_nt_kernel<"),
    "splitk-ws-resid": (0, 300, 256, 2048, 0, 0, 0, "resid", "gemm_bf16_kernel<128, 128,"),
    "splitk-ws-tail-rows-acc": (0, 300, 256, 2048, 32, 0, 100, "acc", "gemm_bf16_kernel<128, 128,"),
}


def gemm_inputs(M, N, K, K2, group, tail_rows, mode, device):
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K + K2 + group + tail_rows + len(mode))
    bf = lambda t: t.bfloat16().to(device)
    inp = dict(a=bf(torch.randn(M, K, generator=g)), w=bf(torch.randn(N, K, generator=g) / K ** 0.5),
               alpha=1.0 if mode == "acc" else 0.75)
    if K2:
        ng = N // group if group else 1
        inp["a2"] = bf(torch.randn(tail_rows or M, K2 * ng, generator=g))
        inp["w2"] = bf(torch.randn(N, K2, generator=g) / 6)
    if mode in ("bias", "resid"):
        inp["bias"] = bf(torch.randn(N, generator=g))
    if mode == "resid":
        inp["resid"] = bf(torch.randn(M, N, generator=g))
    if mode == "acc":
        inp["base"] = torch.randn(M, N, generator=g).to(device)
    return inp


def gemm_reference(inp, group, tail_rows, mode):
    """fp64 reference and the element-wise bound
        u_out |ref| + (K + K2 + 8) 2^-23 (|alpha| (|a| |w|^T + |a2| |w2|^T) + |bias| + |resid|)
    with u_out = 2^-8 for a bf16 output and 2^-23 for an fp32 one (its own rounding).  A bf16 output with a
    residual gets one more 2^-8 |alpha acc + bias|: the residual is added to the bf16-ROUNDED projection, as the unfused
    Linear + add of the reference framework does (gemm.hip "bf16 out: out = bf16(bf16(y) + resid)", gemm8p.hip
    EPI_NONE) -- a documented rounding of the operation, not of its implementation."""
    a, w = inp["a"].double(), inp["w"].double()
    alpha = inp["alpha"]
    M, K = a.shape
    N = w.shape[0]
    y = a @ w.t()
    mag = a.abs() @ w.abs().t()
    K2 = 0
    if "a2" in inp:
        a2, w2 = inp["a2"].double(), inp["w2"].double()
        K2 = w2.shape[1]
        tr = tail_rows or M
        ng = N // group if group else 1
        for j in range(ng):
            cs = slice(j * group, (j + 1) * group) if group else slice(0, N)
            y[:tr, cs] += a2[:, K2 * j:K2 * (j + 1)] @ w2[cs].t()
            mag[:tr, cs] += a2[:, K2 * j:K2 * (j + 1)].abs() @ w2[cs].abs().t()
    proj = alpha * y
    mag = abs(alpha) * mag
    if "bias" in inp:
        proj = proj + inp["bias"].double()
        mag = mag + inp["bias"].double().abs()
    ref = proj
    if "resid" in inp:
        ref = proj + inp["resid"].double()
        mag = mag + inp["resid"].double().abs()
    if mode == "acc":
        ref = proj + inp["base"].double()
        mag = mag + inp["base"].double().abs()
    bound = (U32 if mode == "acc" else U16) * ref.abs() + (K + K2 + 8) * U32 * mag
    if "resid" in inp:
        bound = bound + U16 * proj.abs()
    return ref, bound


def gemm_restatement(inp, group, tail_rows, mode):
    """The documented computation in torch: fp32 products and sums, bf16 output rounding (before and after the residual),
    fp32 accumulate."""
    a, w = inp["a"].float(), inp["w"].float()
    M, N = a.shape[0], w.shape[0]
    y = a @ w.t()
    if "a2" in inp:
        a2, w2 = inp["a2"].float(), inp["w2"].float()
        K2 = w2.shape[1]
        tr = tail_rows or M
        ng = N // group if group else 1
        for j in range(ng):
            cs = slice(j * group, (j + 1) * group) if group else slice(0, N)
            y[:tr, cs] += a2[:, K2 * j:K2 * (j + 1)] @ w2[cs].t()
    y = inp["alpha"] * y
    if "bias" in inp:
        y = y + inp["bias"].float()
    if mode == "acc":
        return inp["base"] + y
    y = y.bfloat16()
    if "resid" in inp:
        y = (y.float() + inp["resid"].float()).bfloat16()
    return y
