"""Shared pieces of the localised-error parity tests (a plain module: no fixtures, no hooks).

Why it exists: a whole-tensor Frobenius ratio ||a - b|| / ||b|| cannot see an error confined to one query row of one
head, one 4-element store chunk or the last key of a ragged tile -- the errors a tiled kernel makes -- and a fresh
contiguous output tensor cannot show a store that lands beside the slice it was meant for.  So:

  rowwise_rel      worst per-(row, 64-wide group) relative error, with its index
  guarded          output views inside a buffer whose every other element must keep its fill pattern, bit for bit
  attention_model  the attention kernels' documented roundings restated in plain torch (sets the per-row bound)
  attention_fp64   the reference
  geglu_* / gemm_* cases, fp64 references and derived element-wise bounds of the GEMM epilogue tests
  group_norm_* / layer_norm_* / norm_*  fp64 references, rounding models, edge-weighted inputs and derived bounds of
                   the norm kernels, saved statistics and parameter gradients included
  conv_*           cases, inputs inside NaN margins, the fp64 reference from torch's own operators with its derived
                   element-wise bound, and a gather restatement (with plantable faults) of every convolution path

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


def guarded_pitch(widths, gap=8):
    """The row pitch (elements) of guarded()'s buffer."""
    return -(-(gap + sum(w + gap for w in widths)) // 8) * 8


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
    ld = guarded_pitch(widths, gap)
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


def guarded_flat(n, dtype=None, device=None, pad=4096):
    """guarded() for an output that has to be dense (the direct small-Cout convolution needs ldo == Cout): one 1-D buffer
    of pad + n + pad elements of the fill pattern.  Returns (view, check): the contiguous n-element view in its middle
    (16-byte aligned: pad is a multiple of 8) and a closure asserting that head and tail kept the fill."""
    if dtype is None:
        from pairwise_sample_optimization_amd import kernels as K
        dtype = K.ELEM
    assert pad % 8 == 0
    size = torch.empty((), dtype=dtype).element_size()
    fill, ivt = FILL_BITS[size], _IVIEW[size]
    buf = torch.empty(pad + n + pad, dtype=dtype, device=device)
    ibuf = buf.view(ivt)
    ibuf.fill_(fill)

    def check(what="guard band"):
        touched = ibuf != fill
        touched[pad:pad + n] = False
        if bool(touched.any()):
            i = int(touched.nonzero()[0])
            where = f"{pad - i} element(s) before the view" if i < pad else f"{i - pad - n} element(s) past its end"
            raise AssertionError(f"{what}: {int(touched.sum())} element(s) outside the {n}-element view were written; "
                                 f"first at {i} of the {pad + n + pad}-element buffer ({where}), bits "
                                 f"{int(ibuf[i]) & (2 ** (8 * size) - 1):#x}")

    return buf[pad:pad + n], check


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


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm (norm.hip) and the ordered LayerNorm parameter gradients (pso_layer_norm_dparam_ws)
# ----------------------------------------------------------------------------------------------------------------------
# What the norm tests hold a kernel to, all of it from the reference side:
#   saved statistics  |mean - mean64| <= F 2^-23 mean|x|  and  |rstd / rstd64 - 1| <= F 2^-23 (E[x^2] + eps) / (var + eps)
#                     per group / row.  (E[x^2] + eps) / (var + eps) is the cancellation amplification of the two-moment
#                     form var = E[x^2] - mean^2: ~1 for centred data, ~1000 at mean / std = 32.
#   y, dx             rowwise_rel(got, ref64, 8) -- one 16-byte store chunk, the unit every norm kernel writes --
#                     within ROW_BOUND_FACTOR x the worst chunk of the rounding model on the same inputs
#   dgamma, dbeta     element-wise F2 2^-23 sum|dz xhat| and F2 2^-23 sum|dz| (+ 2^-23 |previous contents|)
NORM_EPS = 1e-5
GN_ROWS, GN_ROWS_BIG = 64, 512   # pixel rows per block; the forward's above 256 blocks per image (norm.hip)
LN_DPARAM_ROWS = 64              # CS2_ROWS of fullgrad.hip
EDGE_SCALE = 32.0
ELEM_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# F and F2 are NOT taken from a kernel run: tests/test_parity_util.py restates the sums in fp32 with the kernels' own
# sequential chain lengths (gn_partial_kernel: a thread's pixel rows, then the RS row slots, then the Cg channels of a
# group; ln_*_kernel: a lane's 8 * MAXV channels, then the 64-lane butterfly; the dparam kernels: a thread's rows, the
# row slices, the ordered levels), takes the worst error over every named case in bf16 and fp16 in units of the
# expressions above, and checks that each constant is 4 x that worst, rounded up to a power of two and no smaller than
# 8.  Measured worst ratios (CPU restatement):
#   statistics       mean 0.495 units, rstd 2.393 units                       -> F  = 16
#   dgamma / dbeta   377.4 units over all named cases (the shifted GN case)   -> F2 = 2048
#                    9.36 units over all of them but the shifted one          -> F2 (centred) = 64
# Why two F2: xhat is proportional to rstd, so the error the statistics bound ALLOWS rstd -- F x the amplification,
# ~1000 units at mean / std = 32 -- goes straight into dgamma; only the shifted case has it.  NORM_F2 is what the rule
# gives over all named cases and is what the shifted case is held to; every other case is held to NORM_F2_CENTRED, the
# same rule without that case, which implies NORM_F2.  (9 units, not 1: silu'(z) = sg (1 + z (1 - sg)) loses
# |z| 2^-24 in 1 - sg, and the edge rows reach |z| ~ 15.)
NORM_F = 16.0
NORM_F2 = 2048.0
NORM_F2_CENTRED = 64.0

# (B, HW, C, G)
GN_CASES = [
    (2, 100, 320, 32),     # Cg = 10 straddles the 8-channel chunks; ragged second block of 36 rows
    (1, 130, 1920, 32),    # SDXL's concatenated width, a 480-thread block, three blocks
    (2, 70, 960, 32),      # the other concatenated width, 480 threads
    (2, 70, 32, 32),       # Cg = 1
    (2, 70, 64, 1),        # Cg = C
    (1, 65, 8, 1),         # one thread per pixel row, 512 row slots
    (1, 65, 4096, 32),     # the C limit: one row slot, 512 threads
    (1, 70, 264, 33),      # a 264-thread block: no multiple of 64
    (1, 16384, 32, 32),    # 256 blocks of 64 rows: the last size on GN_ROWS in the forward
    (1, 16500, 128, 32),   # the GN_ROWS_BIG forward, ragged last block of 116 rows (the backward stays on 64)
]
GN_SHIFTED_CASE = (2, 100, 320, 32)   # x = 8 + 0.25 randn: the amplification term of the rstd bound at ~1000
GN_NOAFFINE_CASE = (2, 100, 320, 32)  # gamma = beta = None
# dgamma / dbeta reduction regimes of pso_group_norm_bwd at C = 64: BK = B * HW / 64 row blocks, S = BK >= 64 ? 32 :
# BK / 2 splits, the single pass below S = 2.  (B, HW) -> BK = 1, 3 (single pass), 4, 5 (2 splits, ragged), 63 (31
# splits, ragged), 64 (32 splits)
GN_DPARAM_CASES = [(1, 64), (3, 64), (2, 128), (5, 64), (3, 1344), (2, 2048)]
# (M, C): the MAXV 1 -> 2 -> 4 edges at C = 512 / 520 and 1024 / 1032, the smallest and the largest C, M < 4 (one
# workgroup holds 4 rows), and more than one workgroup
LN_CASES = [(5, 8), (3, 320), (7, 512), (7, 520), (6, 1024), (6, 1032), (9, 1280), (5, 2048), (1, 640), (2, 640),
            (3, 640), (300, 640)]
# (M, C, strided): one row; one row into a second block; the scalar tail (C % 8 != 0); 49 row blocks -> two-level
# reduction, splits of 25 and 24; 66 row blocks -> splits of 22; row-strided x / dy
LN_DPARAM_CASES = [(1, 640, False), (65, 640, False), (777, 12, False), (130, 100, False), (3100, 8, False),
                   (4200, 320, False), (130, 640, True)]


def _elem(dtype):
    if dtype is None:
        from pairwise_sample_optimization_amd import kernels as K
        return K.ELEM
    return dtype


def _seed(*ns):
    s = 12345
    for n in ns:
        s = (s * 1000003 + int(n)) % 2147483647
    return s


def gn_rows_fwd(HW):
    return GN_ROWS_BIG if -(-HW // GN_ROWS) > 256 else GN_ROWS


def gn_slots(C):
    """RS of norm.hip's gn_block: row slots of a block of (C / 8) * RS <= 512 threads."""
    tpr, rs = C // 8, 1
    while tpr * rs * 2 <= 512:
        rs *= 2
    return rs


def gn_edge_rows(HW):
    """The pixel rows where a tiling mistake bites: first and last of the image, either side of the first 64-row block
    boundary, and either side of the first 512-row one where the forward takes GN_ROWS_BIG."""
    rows = {0, GN_ROWS - 1, GN_ROWS, HW - 1}
    if gn_rows_fwd(HW) == GN_ROWS_BIG:
        rows |= {GN_ROWS_BIG - 1, GN_ROWS_BIG}
    return sorted(r for r in rows if 0 <= r < HW)


def norm_inputs(kind, shape, dtype=None, device="cpu", shifted=False):
    """x, dy, dadd, gamma, beta of one norm case in the element type, drawn on the CPU from a seed derived from the
    shape (the CPU self-test and the GPU tests see the same numbers).  kind "gn": shape (B, HW, C, G), tensors
    [B, HW, C]; kind "ln": shape (M, C), tensors [M, C].

    Edge-weighted: the edge rows (gn_edge_rows; for LN the channels 0 and C - 1) are scaled by 32 in x and dy, so a
    dropped, doubled or misattributed edge row moves its group's statistics and coefficients by tens of percent, not
    by 1 / HW.  shifted: x = 8 + 0.25 randn with no edge weight on x (mean / std ~ 32 is the point of that case)."""
    et = _elem(dtype)
    g = torch.Generator().manual_seed(_seed(len(kind), int(shifted), *shape))
    if kind == "gn":
        B, HW, C, _ = shape
        x, dy, dadd = (torch.randn(B, HW, C, generator=g) for _ in range(3))
        rows = gn_edge_rows(HW)
        dy[:, rows] *= EDGE_SCALE
        if shifted:
            x = 8.0 + 0.25 * x
        else:
            x[:, rows] *= EDGE_SCALE
    else:
        M, C = shape
        x, dy, dadd = (torch.randn(M, C, generator=g) for _ in range(3))
        x[:, [0, C - 1]] *= EDGE_SCALE
        dy[:, [0, C - 1]] *= EDGE_SCALE
    gamma = 1.0 + 0.25 * torch.randn(C, generator=g)
    beta = 0.25 * torch.randn(C, generator=g)
    return {k: v.to(et).to(device) for k, v in dict(x=x, dy=dy, dadd=dadd, gamma=gamma, beta=beta).items()}


def _silu_parts(z):
    sg = torch.sigmoid(z)
    return z * sg, sg * (1 + z * (1 - sg))   # silu(z), silu'(z)


def gn_reference(x, gamma, beta, G, eps, silu, dy=None, dadd=None):
    """Everything the GroupNorm tests need from fp64, computed from the 16-bit inputs with nothing rounded: y, stats
    [B, G, 2], dx, dgamma, dbeta, and the magnitudes the bounds are made of -- absx = mean|x|, ex2 = E[x^2], var per
    group ([B, G]); mag_g = sum|dz xhat|, mag_b = sum|dz| per channel."""
    B, HW, C = x.shape
    Cg = C // G
    xd = x.double().reshape(B, HW, G, Cg)
    mean = xd.mean((1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    one = torch.ones(C, dtype=torch.float64, device=x.device)
    gm = (gamma.double() if gamma is not None else one).reshape(1, 1, G, Cg)
    bt = (beta.double() if beta is not None else 0 * one).reshape(1, 1, G, Cg)
    xh = (xd - mean) * rstd
    z = xh * gm + bt
    r = dict(y=(_silu_parts(z)[0] if silu else z).reshape(B, HW, C),
             stats=torch.stack([mean.reshape(B, G), rstd.reshape(B, G)], -1), eps=eps,
             absx=xd.abs().mean((1, 3)), ex2=(xd * xd).mean((1, 3)), var=var.reshape(B, G),
             dx=None, dgamma=None, dbeta=None)
    if dy is not None:
        dz = dy.double().reshape(B, HW, G, Cg)
        if silu:
            dz = dz * _silu_parts(z)[1]
        gd = dz * gm
        a = gd.mean((1, 3), keepdim=True)
        b = (gd * xh).mean((1, 3), keepdim=True)
        dx = (rstd * (gd - a - xh * b)).reshape(B, HW, C)
        r.update(dx=dx + dadd.double() if dadd is not None else dx,
                 dgamma=(dz * xh).sum((0, 1)).reshape(C), dbeta=dz.sum((0, 1)).reshape(C),
                 mag_g=(dz * xh).abs().sum((0, 1)).reshape(C), mag_b=dz.abs().sum((0, 1)).reshape(C))
    return r


def group_norm_fp64(x, gamma, beta, G, eps, silu, dy=None, dadd=None):
    """(y, stats[B, G, 2], dx, dgamma, dbeta) in fp64 (the last three None without dy); gamma / beta may be None."""
    r = gn_reference(x, gamma, beta, G, eps, silu, dy, dadd)
    return r["y"], r["stats"], r["dx"], r["dgamma"], r["dbeta"]


def ln_reference(x, gamma, beta, eps, dy=None, dadd=None):
    """gn_reference's LayerNorm twin: per-row statistics [M, 2]; dz = dy (no activation is fused)."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (xd - mean) * rstd
    gm, bt = gamma.double(), beta.double()
    r = dict(y=xh * gm + bt, stats=torch.cat([mean, rstd], 1), eps=eps, absx=xd.abs().mean(1), ex2=(xd * xd).mean(1),
             var=var.reshape(-1), dx=None, dgamma=None, dbeta=None)
    if dy is not None:
        dyd = dy.double()
        gd = dyd * gm
        a = gd.mean(1, keepdim=True)
        b = (gd * xh).mean(1, keepdim=True)
        dx = rstd * (gd - a - xh * b)
        r.update(dx=dx + dadd.double() if dadd is not None else dx, dgamma=(dyd * xh).sum(0), dbeta=dyd.sum(0),
                 mag_g=(dyd * xh).abs().sum(0), mag_b=dyd.abs().sum(0))
    return r


def ln_dparam_reference(x, dy, stats):
    """pso_layer_norm_dparam's own reference: its inputs are x, dy AND the fp32 statistics, so the fp64 sums are taken
    with the statistics it is handed (with fp64 ones, their fp32 rounding -- an input rounding, 2^-24 |mean| against
    an |x - mean| that may be far smaller -- would be charged to the kernel; at M = 1 nothing averages it out).
    Returns dgamma, dbeta and the bound's magnitudes mag_g, mag_b."""
    t = dy.double() * (x.double() - stats[:, :1].double()) * stats[:, 1:].double()
    return dict(dgamma=t.sum(0), dbeta=dy.double().sum(0), mag_g=t.abs().sum(0), mag_b=dy.double().abs().sum(0))


def layer_norm_fp64(x, gamma, beta, eps, dy, dadd):
    """(y, stats[M, 2], dx, dgamma, dbeta) in fp64."""
    r = ln_reference(x, gamma, beta, eps, dy, dadd)
    return r["y"], r["stats"], r["dx"], r["dgamma"], r["dbeta"]


# ---- the rounding models: norm.hip's documented roundings in plain torch fp32 ----------------------------------------
def gn_chunk_sums(v, rows):
    """fp32 per-channel sums of v [B, HW, C] (fp32) over blocks of `rows` pixel rows -> [B, blocks, C]: what one
    workgroup of gn_partial_kernel leaves in its workspace row (torch's summation order, not the kernel's; the ragged
    last block is padded with zeros, which add exactly)."""
    B, HW, C = v.shape
    nch = -(-HW // rows)
    v = torch.nn.functional.pad(v, (0, 0, 0, nch * rows - HW))
    return v.reshape(B, nch, rows, C).sum(2)


def gn_group_combine(ch, G):
    """per-channel block sums [B, blocks, C] fp32 -> fp32 sum over the Cg channels of a group, then gn_finalize_kernel's
    fp64 combine over the blocks -> [B, G] fp64."""
    B, nch, C = ch.shape
    return ch.reshape(B, nch, G, C // G).sum(3).double().sum(1)


def gn_stats_from_sums(a, q, n, eps):
    """gn_finalize_kernel<false>: mean = a / n, var = q / n - mean^2 clamped at 0, both in fp64; (mean, rstd) rounded to
    fp32 -> [B, G, 2]."""
    mean = a / n
    var = (q / n - mean * mean).clamp_min(0.0)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1).float()


def _per_channel(t, Cg):
    return t.repeat_interleave(Cg, 1).unsqueeze(1)   # [B, G] -> [B, 1, C]


def _gn_dz(xf, dy, stats, gm, bt, Cg, silu):
    """xhat and dz = dy silu'(z) as gn_apply_bwd_kernel forms them from fp32 (mean, rstd): xhat = x rstd - mean rstd,
    z = x (rstd gamma) + (beta - mean rstd gamma)."""
    mean, rstd = _per_channel(stats[..., 0], Cg), _per_channel(stats[..., 1], Cg)
    xh = xf * rstd + (-mean * rstd)
    dz = dy.float()
    if silu:
        z = xf * (rstd * gm) + (bt - mean * rstd * gm)
        dz = dz * _silu_parts(z)[1]
    return xh, dz


def gn_model_coef(x, dy, stats, gamma, beta, G, silu):
    """The backward's fp32 group coefficients (mean(dz gamma), mean(dz gamma xhat)) [B, G, 2] from fp32 64-row block
    sums, and the per-channel block sums [B, blocks, C] of dz and dz xhat that dbeta / dgamma are added up from."""
    B, HW, C = x.shape
    Cg = C // G
    gm = gamma.float() if gamma is not None else torch.ones(C, device=x.device)
    bt = beta.float() if beta is not None else torch.zeros(C, device=x.device)
    xh, dz = _gn_dz(x.float(), dy, stats, gm, bt, Cg, silu)
    c1, c2 = gn_chunk_sums(dz, GN_ROWS), gn_chunk_sums(dz * xh, GN_ROWS)
    n = float(HW * Cg)
    coef = torch.stack([gn_group_combine(c1 * gm, G) / n, gn_group_combine(c2 * gm, G) / n], -1).float()
    return coef, c1, c2


def group_norm_model(x, gamma, beta, G, eps, silu, dy=None, dadd=None, stats=None, coef=None):
    """norm.hip's GroupNorm in plain torch: fp32 sums of x and x^2 per block of pixel rows and group, an fp64 combine
    over the blocks, var = E[x^2] - mean^2 clamped at 0, statistics rounded to fp32, y = silu?(x (rstd gamma) +
    (beta - mean rstd gamma)) rounded to the element type; dx = P dz + Q + R xhat (+ dadd) with P = rstd gamma,
    Q = -rstd mean(dz gamma), R = -rstd mean(dz gamma xhat) from fp32 block sums, rounded to the element type; dgamma /
    dbeta the fp64 sum of the fp32 per-channel block sums, rounded to fp32.  Returns (y, stats, dx, dgamma, dbeta).
    stats / coef: use these instead of the model's own (the self-test's wrong restatements)."""
    B, HW, C = x.shape
    Cg = C // G
    et = x.dtype
    xf = x.float()
    if stats is None:
        rows = gn_rows_fwd(HW)
        stats = gn_stats_from_sums(gn_group_combine(gn_chunk_sums(xf, rows), G),
                                   gn_group_combine(gn_chunk_sums(xf * xf, rows), G), float(HW * Cg), eps)
    gm = gamma.float() if gamma is not None else torch.ones(C, device=x.device)
    bt = beta.float() if beta is not None else torch.zeros(C, device=x.device)
    mean, rstd = _per_channel(stats[..., 0], Cg), _per_channel(stats[..., 1], Cg)
    z = xf * (rstd * gm) + (bt - mean * rstd * gm)
    y = (_silu_parts(z)[0] if silu else z).to(et)
    if dy is None:
        return y, stats, None, None, None
    own, c1, c2 = gn_model_coef(x, dy, stats, gamma, beta, G, silu)
    coef = own if coef is None else coef
    xh, dz = _gn_dz(xf, dy, stats, gm, bt, Cg, silu)
    ca, cb = _per_channel(coef[..., 0], Cg), _per_channel(coef[..., 1], Cg)
    dx = (rstd * gm) * dz + ((-rstd * cb) * xh + (-rstd * ca))
    if dadd is not None:
        dx = dx + dadd.float()
    return y, stats, dx.to(et), c2.double().sum((0, 1)).float(), c1.double().sum((0, 1)).float()


def layer_norm_model(x, gamma, beta, eps, dy=None, dadd=None):
    """norm.hip's LayerNorm in plain torch fp32: mean, then a centred variance and rsqrt; y = (x - mean) rstd gamma +
    beta; dx = rstd (g - a - xhat b) + dadd with g = dy gamma, a = mean(g), b = mean(g xhat); outputs rounded to the
    element type.  dgamma / dbeta as ln_dparam_part_kernel forms the terms: dy (x - mean) rstd and dy, summed in fp32.
    Returns (y, stats[M, 2], dx, dgamma, dbeta)."""
    M, C = x.shape
    et = x.dtype
    xf, gf, bf = x.float(), gamma.float(), beta.float()
    mean = xf.sum(1, keepdim=True) / C
    d = xf - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) / C + eps)
    y = (d * rstd * gf + bf).to(et)
    stats = torch.cat([mean, rstd], 1)
    if dy is None:
        return y, stats, None, None, None
    xh = d * rstd
    gd = dy.float() * gf
    a = gd.sum(1, keepdim=True) / C
    b = (gd * xh).sum(1, keepdim=True) / C
    dx = rstd * (gd - a - xh * b)
    if dadd is not None:
        dx = dx + dadd.float()
    return y, stats, dx.to(et), (dy.float() * d * rstd).sum(0), dy.float().sum(0)


# ---- the same sums in the kernels' own order (the self-test derives F and F2 from these) ------------------------------
def _seq_sum(v, dim):
    """Left-to-right fp32 sum along `dim`, one rounded add per element, starting from 0 as the kernels' accumulators do."""
    acc = torch.zeros_like(v.select(dim, 0))
    for i in range(v.shape[dim]):
        acc = acc + v.select(dim, i)
    return acc


def gn_chunk_sums_kernel_order(v, rows):
    """gn_chunk_sums with gn_partial_kernel's chains: row slot s of RS adds the block's rows s, s + RS, ... in order,
    then the RS slots are added in order."""
    B, HW, C = v.shape
    rs = gn_slots(C)
    nch, per = -(-HW // rows), -(-rows // rs)
    v = torch.nn.functional.pad(v, (0, 0, 0, nch * rows - HW)).reshape(B, nch, rows, C)
    v = torch.nn.functional.pad(v, (0, 0, 0, per * rs - rows)).reshape(B, nch, per, rs, C)
    return _seq_sum(_seq_sum(v, 2), 2)


def gn_group_combine_kernel_order(ch, G):
    B, nch, C = ch.shape
    return _seq_sum(ch.reshape(B, nch, G, C // G), 3).double().sum(1)


def gn_kernel_order(x, gamma, beta, G, eps, silu, dy):
    """(stats, dgamma, dbeta) with every fp32 sum in the kernels' order: the forward's statistics, and the backward's
    per-channel sums from those statistics (the single-pass and the split dparam reductions both add the block sums in
    fp64, where the order no longer shows)."""
    B, HW, C = x.shape
    Cg = C // G
    xf = x.float()
    rows = gn_rows_fwd(HW)
    stats = gn_stats_from_sums(gn_group_combine_kernel_order(gn_chunk_sums_kernel_order(xf, rows), G),
                               gn_group_combine_kernel_order(gn_chunk_sums_kernel_order(xf * xf, rows), G),
                               float(HW * Cg), eps)
    gm = gamma.float() if gamma is not None else torch.ones(C)
    bt = beta.float() if beta is not None else torch.zeros(C)
    xh, dz = _gn_dz(xf, dy, stats, gm, bt, Cg, silu)
    c1, c2 = gn_chunk_sums_kernel_order(dz, GN_ROWS), gn_chunk_sums_kernel_order(dz * xh, GN_ROWS)
    return stats, c2.double().sum((0, 1)).float(), c1.double().sum((0, 1)).float()


def _lane_sum(v):
    """One wave's sum as ln_*_kernel takes it: v [M, C] fp32, lane l holds the 8-channel chunks l, l + 64, ... and adds
    their elements in order; then the xor butterfly over the 64 lanes (32, 16, ... 1: a balanced tree)."""
    M, C = v.shape
    c8 = C // 8
    maxv = -(-c8 // 64)
    v = torch.nn.functional.pad(v.reshape(M, c8, 8), (0, 0, 0, maxv * 64 - c8)).reshape(M, maxv, 64, 8)
    s = _seq_sum(v.permute(0, 2, 1, 3).reshape(M, 64, maxv * 8), 2)
    w = 32
    while w:
        s = s[:, :w] + s[:, w:2 * w]
        w //= 2
    return s   # [M, 1]


def ln_stats_kernel_order(x, eps):
    xf = x.float()
    C = x.shape[1]
    mean = _lane_sum(xf) / C
    d = xf - mean
    return torch.cat([mean, torch.rsqrt(_lane_sum(d * d) / C + eps)], 1)


def ln_dparam_plan(M):
    """ordered_reduce_plan of fullgrad.hip for the M / 64 row blocks: (row blocks, splits, blocks per split)."""
    nb = -(-M // LN_DPARAM_ROWS)
    if nb <= 48:
        return nb, nb, 1
    S = min(64, max(1, (nb + 31) // 32))
    ch = -(-nb // S)
    return nb, -(-nb // ch), ch


def ln_dparam_kernel_order(x, dy, stats, prev_g, prev_b):
    """pso_layer_norm_dparam_ws in its own order: a thread adds rows r0 + ty, r0 + ty + 4, ... of its 64-row block, the
    4 slices are added in order, the blocks of a split in order, the splits in order, then out += acc."""
    M, C = x.shape
    nb, S, ch = ln_dparam_plan(M)
    d = dy.float()
    t = torch.stack([d * (x.float() - stats[:, :1]) * stats[:, 1:], d], 0)               # [2, M, C]
    t = torch.nn.functional.pad(t, (0, 0, 0, nb * LN_DPARAM_ROWS - M)).reshape(2, nb, LN_DPARAM_ROWS // 4, 4, C)
    part = _seq_sum(t, 2)
    part = ((part[:, :, 0] + part[:, :, 1]) + part[:, :, 2]) + part[:, :, 3]              # [2, nb, C]
    if ch > 1:
        part = _seq_sum(torch.nn.functional.pad(part, (0, 0, 0, S * ch - nb)).reshape(2, S, ch, C), 2)
    acc = _seq_sum(part, 1)
    return prev_g + acc[0], prev_b + acc[1]


# ---- bounds and checks ------------------------------------------------------------------------------------------------
def norm_stats_units(stats, ref):
    """Worst error of saved statistics [..., 2] against gn_reference / ln_reference, per group or row, in units of
    2^-23 mean|x| (the mean) and of 2^-23 (E[x^2] + eps) / (var + eps) (rstd, relative): (mean_units, rstd_units).  The
    bound is NORM_F units.  A NaN comes back as NaN, which fails `<=`."""
    em = (stats[..., 0].double() - ref["stats"][..., 0]).abs() / (U32 * ref["absx"]).clamp_min(_TINY)
    er = (stats[..., 1].double() / ref["stats"][..., 1] - 1).abs() / (U32 * (ref["ex2"] + ref["eps"])
                                                                        / (ref["var"] + ref["eps"]))
    return em.max().item(), er.max().item()


def norm_dparam_bounds(ref, prevs, f2=None):
    """(dgamma bound, dbeta bound) [C]: f2 2^-23 sum|dz xhat| and f2 2^-23 sum|dz| (f2: NORM_F2_CENTRED unless given),
    plus 2^-23 |previous contents| (prevs: {"dgamma": ..., "dbeta": ...}, either may be missing) where the kernel adds
    to them."""
    out = []
    f2 = NORM_F2_CENTRED if f2 is None else f2
    for name, mag in (("dgamma", "mag_g"), ("dbeta", "mag_b")):
        b = f2 * U32 * ref[mag]
        out.append(b + U32 * prevs[name].double().abs() if name in prevs else b)
    return tuple(out)


def norm_dparam_units(got, ref, prevs):
    """{name: worst error} of the parameter gradients in `got` ({"dgamma": ..., "dbeta": ...}, either may be missing)
    in units of 2^-23 sum|dz xhat| / 2^-23 sum|dz|; previous contents are added to the reference first and their
    rounding allowance 2^-23 |prev| is taken off the error.  The bound is NORM_F2_CENTRED (shifted: NORM_F2) units."""
    out = {}
    for name, mag in (("dgamma", "mag_g"), ("dbeta", "mag_b")):
        if name not in got:
            continue
        prev = prevs[name].double() if name in prevs else torch.zeros_like(ref[name])
        err = (got[name].double() - (ref[name] + prev)).abs() - U32 * prev.abs()
        out[name] = (err / (U32 * ref[mag]).clamp_min(_TINY)).max().item()
    return out


def _vec_violations(got, ref, bound):
    return violations(got.reshape(1, -1), ref.reshape(1, -1), bound.reshape(1, -1))


def norm_chunk_bounds(model, ref):
    """worst 8-chunk of the model's y and dx against fp64: ROW_BOUND_FACTOR x these are the kernels' bounds."""
    return {"y": rowwise_rel(model[0], ref["y"], 8), "dx": rowwise_rel(model[2], ref["dx"], 8)}


def _assert_norm_outputs(tag, got, stats, dparams, ref, model, prevs, f2=None):
    """Assertions 2 - 5 of a norm case (1, the guard bands, is the caller's): finite, statistics, chunks, dparams."""
    worst = norm_chunk_bounds(model, ref)
    mu, ru = norm_stats_units(stats, ref)
    mmu, mru = norm_stats_units(model[1], ref)
    line = [f"{n} kernel {rowwise_rel(t, ref[n], 8)} model {worst[n]}" for n, t in got.items()]
    line.append(f"stats units mean {mu:.2f} rstd {ru:.2f} (model {mmu:.2f} {mru:.2f}, bound {NORM_F:g})")
    if dparams:
        ug = norm_dparam_units(dparams, ref, prevs)
        line.append("dparam units " + " ".join(f"{n} {u:.2f}" for n, u in ug.items())
                    + f" (bound {NORM_F2_CENTRED if f2 is None else f2:g})")
    print(f"\n[norm {tag}] " + "; ".join(line), flush=True)
    for n, t in got.items():
        assert torch.isfinite(t.float()).all(), (tag, n)                                          # 2.
    assert torch.isfinite(stats).all(), (tag, "stats")
    assert mu <= NORM_F and ru <= NORM_F, (f"{tag} stats: mean {mu:.2f}, rstd {ru:.2f} units of the derived bound, "
                                           f"allowed {NORM_F:g}")                                    # 3.
    for n, t in got.items():                                                                      # 4.
        e, bound = rowwise_rel(t, ref[n], 8), ROW_BOUND_FACTOR * worst[n]
        assert e < bound, f"{tag} {n}: worst 8-chunk {e}, bound {bound:.3e} = 3 x model {worst[n]}"
    bg, bb = norm_dparam_bounds(ref, prevs, f2)
    for n, bound in (("dgamma", bg), ("dbeta", bb)):                                              # 5.
        if n in dparams:
            assert torch.isfinite(dparams[n]).all(), (tag, n)
            want = ref[n] + (prevs[n].double() if n in prevs else 0)
            cnt, msg = _vec_violations(dparams[n], want, bound)
            assert cnt == 0, f"{tag} {n}: {msg}"


def _fill_guarded(rows, widths, src, device, gap=8):
    """guarded() views holding copies of the [rows, w] tensors in src; returns (views, check)."""
    views, check = guarded(rows, widths, gap=gap, dtype=src[0].dtype, device=device)
    for v, s in zip(views, src):
        v.copy_(s.reshape(rows, -1))
    return views, check


def run_group_norm_case(cuda, B, HW, C, G, silu, affine=True, shifted=False, accumulate=False,
                        want=("dgamma", "dbeta")):
    """One GroupNorm case of tests/test_gpu_norm_parity.py (and of the fp16 library's in tests/test_gpu_f16.py):
    forward and backward with dadd, inputs that end where the payload NaNs begin, outputs in guarded buffers, fp32
    parameter gradients in guarded buffers over non-zero previous contents, the five assertions."""
    from pairwise_sample_optimization_amd import kernels as K
    tag = f"gn {K.ELEM} {(B, HW, C, G)} silu={silu}" + (" no-affine" if not affine else "") \
        + (" shifted" if shifted else "") + (" accumulate" if accumulate else "") + f" {'+'.join(want)}"
    inp = norm_inputs("gn", (B, HW, C, G), K.ELEM, "cpu", shifted)
    ins, checks = {}, []
    for n in ("x", "dy", "dadd"):   # gap = 0: the row after the last one is fill, so a read past the end shows
        (v,), chk = _fill_guarded(B * HW, [C], [inp[n]], cuda, gap=0)
        ins[n] = v.view(B, HW, C)
        checks.append((n, chk))
    x, dy, dadd = ins["x"], ins["dy"], ins["dadd"]
    gamma, beta = (inp["gamma"].to(cuda), inp["beta"].to(cuda)) if affine else (None, None)
    ref = gn_reference(x, gamma, beta, G, NORM_EPS, silu, dy, dadd)
    model = group_norm_model(x, gamma, beta, G, NORM_EPS, silu, dy, dadd)
    (y2,), chk_y = guarded(B * HW, [C], gap=0, device=cuda)
    (dx2,), chk_dx = guarded(B * HW, [C], gap=0, device=cuda)
    checks += [("y", chk_y), ("dx", chk_dx)]
    gen = torch.Generator().manual_seed(_seed(B, HW, C, G, 7))
    prevs, outs = {}, {}
    for n in want:   # non-zero previous contents either way: without accumulate they must not show
        prev = torch.randn(C, generator=gen).to(cuda)
        (v,), chk = _fill_guarded(1, [C], [prev], cuda)
        outs[n] = v[0]
        checks.append((n, chk))
        if accumulate:
            prevs[n] = prev
    y, stats = K.group_norm_fwd(x, gamma, beta, G, NORM_EPS, silu, out=y2.view(B, HW, C))
    dx = K.group_norm_bwd(x, dy, stats, gamma, beta, silu, dadd=dadd, dgamma=outs.get("dgamma"),
                          dbeta=outs.get("dbeta"), accumulate=accumulate, out=dx2.view(B, HW, C))
    torch.cuda.synchronize()
    assert y.data_ptr() == y2.data_ptr() and dx.data_ptr() == dx2.data_ptr() and stats.shape == (B, G, 2)
    for n, chk in checks:                                                                         # 1.
        chk(f"{tag} {n}")
    for n in ("x", "dy", "dadd"):
        assert torch.equal(ins[n].cpu().view(torch.int16), inp[n].view(torch.int16)), f"{tag}: input {n} was written"
    _assert_norm_outputs(tag, {"y": y, "dx": dx}, stats, outs, ref, model, prevs, NORM_F2 if shifted else None)


def run_layer_norm_case(cuda, M, C):
    """One LayerNorm case: x, dy, dadd column slices of guarded buffers (16-byte aligned, ld > C, three different ld),
    y and dx written into guarded slices through out=, backward with dadd as unet.py calls it, the five assertions
    (dgamma / dbeta have their own cases: run_ln_dparam_case)."""
    from pairwise_sample_optimization_amd import kernels as K
    tag = f"ln {K.ELEM} {(M, C)}"
    inp = norm_inputs("ln", (M, C), K.ELEM, "cpu")
    ins, checks = {}, []
    for n, gap in (("x", 8), ("dy", 16), ("dadd", 24)):
        (v,), chk = _fill_guarded(M, [C], [inp[n]], cuda, gap=gap)
        ins[n] = v
        checks.append((n, chk))
    x, dy, dadd = ins["x"], ins["dy"], ins["dadd"]
    assert len({t.stride(0) for t in (x, dy, dadd)}) == 3 and all(t.stride(0) > C for t in (x, dy, dadd))
    gamma, beta = inp["gamma"].to(cuda), inp["beta"].to(cuda)
    ref = ln_reference(x, gamma, beta, NORM_EPS, dy, dadd)
    model = layer_norm_model(x, gamma, beta, NORM_EPS, dy, dadd)
    (yv,), chk_y = guarded(M, [C], device=cuda)
    (_, dxv), chk_dx = guarded(M, [C, C], device=cuda)   # the second slice: ld = 2 C + 24
    checks += [("y", chk_y), ("dx", chk_dx)]
    y, stats = K.layer_norm_fwd(x, gamma, beta, NORM_EPS, out=yv)
    dx = K.layer_norm_bwd(x, dy, stats, gamma, dadd=dadd, out=dxv)
    torch.cuda.synchronize()
    assert y.data_ptr() == yv.data_ptr() and dx.data_ptr() == dxv.data_ptr() and stats.shape == (M, 2)
    for n, chk in checks:                                                                         # 1.
        chk(f"{tag} {n}")
    for n in ("x", "dy", "dadd"):
        assert torch.equal(ins[n].cpu().view(torch.int16), inp[n].view(torch.int16)), f"{tag}: input {n} was written"
    _assert_norm_outputs(tag, {"y": y, "dx": dx}, stats, {}, ref, model, {})


def run_ln_dparam_case(cuda, M, C, strided):
    """One case of the ordered LayerNorm parameter gradients (K.layer_norm_dparam, the product path): statistics handed
    over as the fp32 rounding of the fp64 ones (ln_dparam_reference is taken with them), dgamma / dbeta in guarded fp32 buffers over non-zero contents (the op
    accumulates); zero violations of the derived bound, and the same bits on a second call."""
    from pairwise_sample_optimization_amd import kernels as K
    tag = f"ln dparam {K.ELEM} {(M, C)}" + (" strided" if strided else "")
    inp = norm_inputs("ln", (M, C), K.ELEM, "cpu")
    if strided:
        (x,), _ = _fill_guarded(M, [C], [inp["x"]], cuda, gap=8)
        (dy,), _ = _fill_guarded(M, [C], [inp["dy"]], cuda, gap=16)
        assert x.stride(0) > C and dy.stride(0) > C and x.stride(0) != dy.stride(0)
    else:
        x, dy = inp["x"].to(cuda), inp["dy"].to(cuda)
    stats = ln_reference(x, inp["gamma"].to(cuda), inp["beta"].to(cuda), NORM_EPS)["stats"].float()
    ref = ln_dparam_reference(x, dy, stats)
    gen = torch.Generator().manual_seed(_seed(M, C, 11))
    prevs = {n: torch.randn(C, generator=gen).to(cuda) for n in ("dgamma", "dbeta")}
    runs = []
    for _ in range(2):
        outs, checks = {}, []
        for n in ("dgamma", "dbeta"):
            (v,), chk = _fill_guarded(1, [C], [prevs[n]], cuda)
            outs[n] = v[0]
            checks.append((n, chk))
        K.layer_norm_dparam(x, dy, stats, outs["dgamma"], outs["dbeta"])
        torch.cuda.synchronize()
        for n, chk in checks:
            chk(f"{tag} {n}")
        runs.append(outs)
    outs = runs[0]
    ug = norm_dparam_units(outs, ref, prevs)
    print(f"\n[norm {tag}] plan (blocks, splits, per split) {ln_dparam_plan(M)}; units dgamma {ug['dgamma']:.2f} dbeta "
          f"{ug['dbeta']:.2f} (bound {NORM_F2_CENTRED:g})", flush=True)
    bg, bb = norm_dparam_bounds(ref, prevs)
    for n, bound in (("dgamma", bg), ("dbeta", bb)):
        assert torch.isfinite(outs[n]).all(), (tag, n)
        cnt, msg = _vec_violations(outs[n], ref[n] + prevs[n].double(), bound)
        assert cnt == 0, f"{tag} {n}: {msg}"
        assert torch.equal(runs[0][n], runs[1][n]), f"{tag} {n}: a second call gave other bits"


# ----------------------------------------------------------------------------------------------------------------------
# convolutions: the implicit GEMM's gather (gemm.hip issue_tile / load_chunk_conv, gemm8p.hip CONV), conv_small.hip
# ----------------------------------------------------------------------------------------------------------------------
CONV_NORMAL, CONV_UP2, CONV_T2 = 1, 2, 3   # kernels.CONV_*; the third template argument of gemm_bf16_kernel


def _tile(bm, bn, conv, wm=2, wn=2, pipe=False):
    """launch()'s pso_note_kernel string of a 2-phase tile (gemm.hip)."""
    return f"gemm_bf16_kernel<{bm}, {bn}, {conv}, {wm}, {wn}, 2, {'true' if pipe else 'false'}, 0>"


_CONV8 = "gemm8p_kernel<0, true, false, false, 320, true>"


def _cc(kind, B, H, W, C1, Cout, mode, kernel, variant=0, C2=0, ks=3, K2=0, out_hw=None, ws=False, ws_ks=0,
        out="guarded"):
    return dict(kind=kind, B=B, H=H, W=W, C1=C1, C2=C2, Cout=Cout, ks=ks, K2=K2, mode=mode, kernel=kernel,
                variant=variant, out_hw=out_hw, ws=ws, ws_ks=ws_ks, out=out)


# id -> geometry (kind, B, H, W of the INPUT, C1 (+ C2), Cout), epilogue mode, variant, kernel name
#   kind:  "s1" stride 1, pad ks // 2; "s2" stride 2, pad 1; "s2asym" stride 2, pad 0, out_hw = (H // 2, W // 2) (the
#          VAE downsample, vae.py); "up2" CONV_UP2; "t2" CONV_T2 with the input dy and out_hw the stride-2 conv's input
#   mode:  "full" bias + rowbias + resid, 16-bit out; "bias" bias only, 16-bit out; "none" 16-bit out, no operand;
#          "f32" fp32 out, no operand; "acc" fp32 accumulate over previous contents
#   ws:    pso_conv2d_ws_bytes > 0, so kernels.conv2d hands pso_conv2d_ws a workspace; ws_ks: the K-splits the plan
#          then takes (variant 52 declines the workspace it is handed: ws without ws_ks)
#   out:   "guarded" a column slice of guarded() (ldo > Cout); "flat" guarded_flat() (ldo == Cout)
# A 9 x 7 image is 63 pixels: 3 images are 189 rows, every 64-row tile holds two images and the last tile is ragged.
# The stride-2 / asymmetric cases have M = 40 / 24 / 30 <= 64 rows at N = 128, where the dispatch takes the 64 x 128
# tile (gemm_plan.h "if (f.M <= 64)"), not 64 x 64: the geometry is kept and the name says what runs.
CONV_CASES = {
    "s1-straddle": _cc("s1", 3, 9, 7, 64, 100, "full", _tile(64, 64, 1)),
    "s1-f32": _cc("s1", 3, 9, 7, 64, 100, "f32", _tile(64, 64, 1)),
    "s1-acc": _cc("s1", 3, 9, 7, 64, 100, "acc", _tile(64, 64, 1)),
    "s1-tail": _cc("s1", 3, 9, 7, 64, 128, "full", _tile(64, 64, 1), K2=32),
    "s1-concat": _cc("s1", 2, 9, 7, 64, 64, "full", _tile(64, 64, 1), C2=128),
    "1x1": _cc("s1", 2, 9, 7, 128, 64, "bias", _tile(64, 64, 1), ks=1),
    "s2-odd": _cc("s2", 2, 9, 7, 64, 128, "full", _tile(64, 128, 1)),
    "s2-even": _cc("s2", 2, 8, 6, 64, 128, "bias", _tile(64, 128, 1)),
    "s2asym-vae": _cc("s2asym", 2, 10, 6, 128, 128, "bias", _tile(64, 128, 1)),
    "up2": _cc("up2", 2, 5, 3, 128, 64, "bias", _tile(64, 64, 2)),
    "t2-odd": _cc("t2", 2, 5, 4, 128, 64, "f32", _tile(64, 64, 3), out_hw=(9, 7)),
    "t2-even": _cc("t2", 2, 4, 3, 128, 64, "f32", _tile(64, 64, 3), out_hw=(8, 6)),
    # 36 K-tiles -> two splits of 18, one 128 x 128 tile; the reduce kernel applies the epilogue once
    "splitk": _cc("s1", 2, 9, 7, 256, 64, "full", _tile(128, 128, 1, 2, 4), ws=True, ws_ks=2),
    "splitk-concat": _cc("s1", 2, 9, 7, 192, 64, "full", _tile(128, 128, 1, 2, 4), C2=64, ws=True, ws_ks=2),
    "small-c1": _cc("s1", 2, 16, 32, 64, 1, "bias", "conv3x3_smallc_kernel<1, 0>", out="flat"),
    "small-c2": _cc("s1", 2, 16, 32, 64, 2, "bias", "conv3x3_smallc_kernel<2, 0>", out="flat"),
    "small-c3": _cc("s1", 2, 16, 32, 64, 3, "bias", "conv3x3_smallc_kernel<3, 0>", out="flat"),
    "small-c3-128": _cc("s1", 2, 32, 16, 128, 3, "none", "conv3x3_smallc_kernel<3, 128>", out="flat"),
    # ldo != Cout: must NOT take the direct kernel -- the N = 3 implicit GEMM
    "small-strided-out": _cc("s1", 2, 16, 32, 64, 3, "bias", _tile(64, 64, 1)),
    # knob-pinned forms (the tools build)
    "8p-one-tile": _cc("s1", 1, 16, 16, 64, 320, "full", _CONV8, variant=44),
    "8p-three-images": _cc("s1", 3, 16, 16, 64, 320, "full", _CONV8, variant=44),
    "8p-wide": _cc("s1", 2, 8, 32, 128, 640, "full", _CONV8, variant=44),
    "8p-tall": _cc("s1", 1, 32, 8, 64, 320, "full", _CONV8, variant=44),
    "tile-256x256": _cc("s1", 3, 9, 7, 64, 320, "full", _tile(256, 256, 1, 2, 4), variant=4),
    "tile-128x160": _cc("s1", 3, 9, 7, 64, 320, "full", _tile(128, 160, 1), variant=12),
    "tile-128x128": _cc("s1", 3, 9, 7, 64, 320, "full", _tile(128, 128, 1, 2, 4), variant=8),
    "tile-64x160": _cc("s1", 3, 9, 7, 64, 320, "full", _tile(64, 160, 1), variant=20),
    "tile-128x128-pipe": _cc("s1", 3, 9, 7, 64, 320, "full", _tile(128, 128, 1, 2, 4, True), variant=11),
    # the splitk shape and inputs with the split off: N = 64 -> the unsplit 64 x 64 tile, held to the same bound
    "splitk-off": _cc("s1", 2, 9, 7, 256, 64, "full", _tile(64, 64, 1), variant=52, ws=True),
}
CONV_DEFAULT_IDS = [k for k, c in CONV_CASES.items() if c["variant"] == 0]
CONV_KNOB_IDS = [k for k, c in CONV_CASES.items() if c["variant"] != 0]
# Worst |conv_restatement - fp64| / bound over every id above, measured by tests/test_parity_util.py on the CPU (it
# prints one line per id): bf16 0.970 ("1x1"), fp16 0.905 ("1x1"); the fp32-output ids stay below 0.002.  Close to 1 is
# what the bound means: u_out is the unit roundoff of the output format, which the final rounding of a value just above
# a power of two reaches; the (K + K2 + 8) 2^-23 term is what is left for the order of the fp32 sums.


def conv_geom(case):
    """(mode, stride, pad, Ho, Wo): the arguments kernels.conv2d is called with (T2 as unet.py calls it: stride and
    pad at their defaults 1 and ks // 2, the target size through out_hw)."""
    kind, H, W, ks = case["kind"], case["H"], case["W"], case["ks"]
    if kind == "s1":
        return CONV_NORMAL, 1, ks // 2, H, W
    if kind == "s2":
        return CONV_NORMAL, 2, 1, (H + 2 - ks) // 2 + 1, (W + 2 - ks) // 2 + 1
    if kind == "s2asym":
        return CONV_NORMAL, 2, 0, H // 2, W // 2
    if kind == "up2":
        return CONV_UP2, 1, 1, 2 * H, 2 * W
    assert kind == "t2", kind
    return CONV_T2, 1, 1, case["out_hw"][0], case["out_hw"][1]


def conv_alpha(case):
    """0.75; 1.0 for accumulate and for the Cout <= 3 cases (the direct small-Cout form needs alpha == 1, and the
    strided-output case must miss that form through its row pitch alone)."""
    return 1.0 if case["mode"] == "acc" or case["Cout"] <= 3 else 0.75


def _nan_margined(t, margin, device):
    """t as the interior of a flat buffer whose `margin` elements either side hold NaN (a tap that leaves the tensor
    reads NaN, not a neighbouring allocation)."""
    n = t.numel()
    buf = torch.full((n + 2 * margin,), float("nan"), dtype=t.dtype)
    buf[margin:margin + n] = t.reshape(-1)
    return buf.to(device)[margin:margin + n].view(t.shape)


def conv_inputs(case, dtype=None, device="cpu"):
    """The operands of one conv case in the element type, drawn on the CPU from a seed derived from the geometry alone
    (so "splitk" and "splitk-off" see the same numbers): x (and x2) NHWC inside NaN margins of at least (W + 2) * C
    elements; w [Cout, ks, ks, C1 + C2] scaled by 1 / (ks sqrt(Ct)); by mode bias [Cout], rowbias [B, Cout], resid
    [B, Ho, Wo, Cout], base (fp32, accumulate); a2 [M, K2] and w2 [Cout, K2] for the LoRA tail; alpha."""
    et = _elem(dtype)
    B, H, W, C1, C2, Cout, ks, K2, mode = (case[k] for k in ("B", "H", "W", "C1", "C2", "Cout", "ks", "K2", "mode"))
    _, _, _, Ho, Wo = conv_geom(case)
    Ct = C1 + C2
    g = torch.Generator().manual_seed(_seed(len(case["kind"]), B, H, W, C1, C2, Cout, ks, K2, Ho, Wo, len(mode)))
    dev = lambda t: t.to(et).to(device)
    inp = dict(x=_nan_margined(torch.randn(B, H, W, C1, generator=g).to(et), (W + 2) * C1, device))
    if C2:
        inp["x2"] = _nan_margined(torch.randn(B, H, W, C2, generator=g).to(et), (W + 2) * C2, device)
    inp["w"] = dev(torch.randn(Cout, ks, ks, Ct, generator=g) / (ks * Ct ** 0.5))
    inp["alpha"] = conv_alpha(case)
    if mode in ("full", "bias"):
        inp["bias"] = dev(torch.randn(Cout, generator=g))
    if mode == "full":
        inp["rowbias"] = dev(torch.randn(B, Cout, generator=g))
        inp["resid"] = dev(torch.randn(B, Ho, Wo, Cout, generator=g))
    if mode == "acc":
        inp["base"] = torch.randn(B, Ho, Wo, Cout, generator=g).to(device)
    if K2:
        inp["a2"] = dev(torch.randn(B * Ho * Wo, K2, generator=g))
        inp["w2"] = dev(torch.randn(Cout, K2, generator=g) / 6)
    return inp


def _conv_torch(xc, wn, case):
    """The case's convolution by torch's own operators: xc [B, Ct, H, W], wn [Cout, Ct, ks, ks] of one float type ->
    [B, Cout, Ho, Wo].  No index formula of the kernels appears here."""
    F = torch.nn.functional
    kind = case["kind"]
    if kind == "s1":
        return F.conv2d(xc, wn, padding=case["ks"] // 2)
    if kind == "s2":
        return F.conv2d(xc, wn, stride=2, padding=1)
    if kind == "s2asym":   # diffusers' Downsample2D of the VAE: pad (0, 1, 0, 1), then a stride-2 conv without padding
        return F.conv2d(F.pad(xc, (0, 1, 0, 1)), wn, stride=2)
    if kind == "up2":
        return F.conv2d(F.interpolate(xc, scale_factor=2, mode="nearest"), wn, padding=1)
    assert kind == "t2", kind
    # the input gradient of y = conv2d(z, w_fwd, stride 2, pad 1) for dy = xc: w_fwd [Co, Ci, kh, kw] is the kernel's
    # unflipped [Ci][kh][kw][Co] weight; linear in dy and w_fwd, so |dy|, |w| give the magnitude
    Ho, Wo = case["out_hw"]
    z = torch.zeros(xc.shape[0], wn.shape[0], Ho, Wo, dtype=xc.dtype, requires_grad=True)
    y = F.conv2d(z, wn.permute(1, 0, 2, 3), stride=2, padding=1)
    assert y.shape == xc.shape, (y.shape, xc.shape)
    (gz,) = torch.autograd.grad(y, z, xc)
    return gz


def _conv_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])   # [B, Cout, Ho, Wo] -> [B * Ho * Wo, Cout]


def conv_reference(inp, case):
    """fp64 reference [M, Cout] and the element-wise bound of one conv case, on the CPU with torch's own operators
    (_conv_torch: F.conv2d, F.pad, F.interpolate, torch.autograd.grad, torch.cat -- not the kernels' index formulae).
    The bound is gemm_reference's with K = ks ks (C1 + C2):
        u_out |ref| + (K + K2 + 8) 2^-23 (|alpha| (conv(|x|, |w|) + |a2| |w2|^T) + |bias| + |rowbias| + |resid or base|)
    u_out = ELEM_ULP of the element type for a 16-bit output, 2^-23 for an fp32 one.  A 16-bit output with a residual
    gets one more u_out |alpha acc + bias + rowbias|: the residual is added to the ROUNDED projection (gemm.hip "bf16
    out: out = bf16(bf16(y) + resid)", the staged epilogue and gemm_splitk_reduce_kernel; gemm8p.hip EPI_NONE) -- a
    documented rounding of the operation.  The magnitude term is the same torch operator on the absolute values."""
    c64 = lambda t: t.detach().cpu().double()
    et = inp["x"].dtype
    x = c64(inp["x"])
    if "x2" in inp:
        x = torch.cat([x, c64(inp["x2"])], -1)
    xc, wn = x.permute(0, 3, 1, 2), c64(inp["w"]).permute(0, 3, 1, 2)
    y = _conv_rows(_conv_torch(xc, wn, case))
    mag = _conv_rows(_conv_torch(xc.abs(), wn.abs(), case))
    M, Cout = y.shape
    K, K2 = case["ks"] * case["ks"] * (case["C1"] + case["C2"]), case["K2"]
    if K2:
        a2, w2 = c64(inp["a2"]), c64(inp["w2"])
        y = y + a2 @ w2.t()
        mag = mag + a2.abs() @ w2.abs().t()
    proj, mag = inp["alpha"] * y, abs(inp["alpha"]) * mag
    if "bias" in inp:
        proj = proj + c64(inp["bias"])
        mag = mag + c64(inp["bias"]).abs()
    if "rowbias" in inp:
        rb = c64(inp["rowbias"]).repeat_interleave(M // case["B"], 0)
        proj, mag = proj + rb, mag + rb.abs()
    ref = proj
    for name in ("resid", "base"):
        if name in inp:
            t = c64(inp[name]).reshape(M, Cout)
            ref, mag = proj + t, mag + t.abs()
    f32_out = case["mode"] in ("f32", "acc")
    u_out = U32 if f32_out else ELEM_ULP[et]
    bound = u_out * ref.abs() + (K + K2 + 8) * U32 * mag
    if "resid" in inp and not f32_out:
        bound = bound + u_out * proj.abs()
    return ref, bound


CONV_FAULTS = ("wrap", "wrap-one-chunk", "replicate", "pad-top-left", "rowbias-tile", "t2-swap", "epilogue-per-split")


def _conv_gather(x, case, fault=None, at=None):
    """The implicit GEMM's A operand [M, ks ks Ct] (tap-major, channel-minor) of x [B, H, W, Ct], by the gather formulae
    of gemm.hip's header (NORMAL iy = oy S + kh - P; UP2 iy = (oy + kh - P) >> 1 inside the 2x grid; T2 iy = (oy + P -
    kh) / 2 where that is even, non-negative and below H), zero where a tap leaves the image.  fault: one of the planted
    gather mistakes of CONV_FAULTS (a wrong bound wraps into the neighbouring row, never out of the image); at: the
    output row oy of "wrap-one-chunk" (default Ho // 2)."""
    mode, stride, pad, Ho, Wo = conv_geom(case)
    B, H, W, Ct = x.shape
    ks = case["ks"]
    if fault == "pad-top-left":   # the asymmetric pad on the top and left instead of the bottom and right
        pad = 1
    oy = torch.arange(Ho).view(Ho, 1).expand(Ho, Wo)
    ox = torch.arange(Wo).view(1, Wo).expand(Ho, Wo)
    flat = x.reshape(B, H * W, Ct)
    cols = []
    for kh in range(ks):
        for kw in range(ks):
            if mode == CONV_NORMAL:
                iy, ix = oy * stride + kh - pad, ox * stride + kw - pad
                oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            elif mode == CONV_UP2:
                uy, ux = oy + kh - pad, ox + kw - pad
                oky, okx = (uy >= 0) & (uy < 2 * H), (ux >= 0) & (ux < 2 * W)
                if fault == "replicate":   # the border pixel again instead of zero
                    uy, ux, oky, okx = uy.clamp(0, 2 * H - 1), ux.clamp(0, 2 * W - 1), oky | True, okx | True
                iy, ix = uy >> 1, ux >> 1
            else:
                ty, tx = oy + pad - kh, ox + pad - kw
                iy, ix = ty >> 1, tx >> 1
                hb, wb = (W, H) if fault == "t2-swap" else (H, W)   # H and W exchanged in the bound
                oky, okx = (ty >= 0) & (ty % 2 == 0) & (iy < hb), (tx >= 0) & (tx % 2 == 0) & (ix < wb)
            ok = oky & okx
            wrapped = torch.zeros_like(ok)
            if fault == "wrap":             # the horizontal bound forgotten: pixel iy W + ix of the neighbouring row
                wrapped = oky & ~okx
            elif fault == "wrap-one-chunk" and (kh, kw) == (1, 0):
                # ... by one lane: one 16-byte chunk of the left tap of one left-edge pixel of the last image
                wrapped[Ho // 2 if at is None else at, 0] = True
            pix = iy * W + ix
            inside = (pix >= 0) & (pix < H * W)
            take = flat[:, pix.clamp(0, H * W - 1).reshape(-1), :]
            g = take * (ok & inside).reshape(1, -1, 1).to(take.dtype)
            if bool(wrapped.any()):
                w_ = (wrapped & inside).reshape(1, -1, 1).to(take.dtype)
                if fault == "wrap-one-chunk":
                    w_ = w_.expand(B, -1, Ct).clone()
                    w_[:B - 1] = 0          # the last image only
                    w_[:, :, 8:] = 0        # channels 0 .. 7: one 16-byte chunk
                g = g + take * w_
            cols.append(g)
    return torch.stack(cols, 2).reshape(B * Ho * Wo, ks * ks * Ct)


def conv_restatement(inp, case, fault=None, at=None):
    """The documented computation in fp32 torch: the gathered patch matrix times the weights with fp32 sums, the LoRA
    tail, alpha, bias, the per-image row bias; a 16-bit output rounded to the element type, and once more after the
    residual; fp32 accumulate onto base.  [M, Cout].  fault: one of CONV_FAULTS, planted for the self-test."""
    assert fault is None or fault in CONV_FAULTS, fault
    c32 = lambda t: t.detach().cpu().float()
    et = inp["x"].dtype
    x = c32(inp["x"])
    if "x2" in inp:
        x = torch.cat([x, c32(inp["x2"])], -1)
    w = c32(inp["w"])
    Cout = w.shape[0]
    y = _conv_gather(x, case, fault, at) @ w.reshape(Cout, -1).t()
    M = y.shape[0]
    if "a2" in inp:
        y = y + c32(inp["a2"]) @ c32(inp["w2"]).t()
    y = inp["alpha"] * y
    times = 2 if fault == "epilogue-per-split" else 1   # every one of the two K-splits adding the epilogue operands
    if "bias" in inp:
        y = y + times * c32(inp["bias"])
    if "rowbias" in inp:
        img = torch.arange(M) // (M // case["B"])
        if fault == "rowbias-tile":   # the second 64-row tile takes its image from its first row
            img[64:128] = img[64]
        y = y + times * c32(inp["rowbias"])[img]
    if case["mode"] == "acc":
        return c32(inp["base"]).reshape(M, Cout) + y
    if case["mode"] == "f32":
        return y
    y = y.to(et)
    if "resid" in inp:
        y = (y.float() + times * c32(inp["resid"]).reshape(M, Cout)).to(et)
    return y


def conv_plan_case(case_id):
    """The case as tests/gemm_plan_cases.py describes a problem (the fields of PsoGemmPlanQuery that differ from its
    defaults), with the operand alignments and row pitches run_conv_case hands over."""
    c = CONV_CASES[case_id]
    mode, stride, pad, Ho, Wo = conv_geom(c)
    full, f32_out = c["mode"] == "full", c["mode"] in ("f32", "acc")
    q = dict(entry="pso_conv2d_ws" if c["ws"] else "pso_conv2d", variant=c["variant"], conv_mode=mode, B=c["B"],
             C1=c["C1"], C2=c["C2"], H=c["H"], W=c["W"], Ho=Ho, Wo=Wo, ks=c["ks"], stride=stride, pad=pad, N=c["Cout"],
             K2=c["K2"], out_dtype=0 if f32_out else 1, accumulate=int(c["mode"] == "acc"),
             alpha=conv_alpha(c),
             bias_align=16 if c["mode"] in ("full", "bias") else 0, rowbias_align=16 if full else 0,
             resid_align=16 if full else 0, out_align=16,
             ldo=c["Cout"] if c["out"] == "flat" else guarded_pitch([c["Cout"]]))
    return q


def run_conv_case(cuda, case_id):
    """One conv case end to end (tests/test_gpu_conv_guarded.py, and the fp16 library's in tests/test_gpu_f16.py): the
    inputs inside NaN margins, the fp64 reference and derived bound from the CPU, the output a guarded column slice (or
    guarded_flat where the form needs a dense one), the kernel name, the guard band, finiteness, zero violations."""
    from pairwise_sample_optimization_amd import kernels as K
    case = CONV_CASES[case_id]
    mode, stride, pad, Ho, Wo = conv_geom(case)
    B, Cout, K2 = case["B"], case["Cout"], case["K2"]
    M, K1 = B * Ho * Wo, case["ks"] * case["ks"] * (case["C1"] + case["C2"])
    inp = conv_inputs(case, K.ELEM, cuda)                                                          # 1.
    ref, bound = conv_reference(inp, case)                                                         # 2.
    f32_out = case["mode"] in ("f32", "acc")
    odt = torch.float32 if f32_out else K.ELEM
    if case["out"] == "flat":                                                                      # 3.
        flat, check = guarded_flat(M * Cout, dtype=odt, device=cuda)
        out = flat.view(B, Ho, Wo, Cout)
        assert out.is_contiguous()
    else:
        (o2,), check = guarded(M, [Cout], dtype=odt, device=cuda)
        out = o2.view(B, Ho, Wo, Cout)
        assert not out.is_contiguous() and out.stride(2) == guarded_pitch([Cout]) > Cout
    if case["mode"] == "acc":                                                                      # 4.
        out.copy_(inp["base"])
    kw = {k: inp[k] for k in ("x2", "bias", "rowbias", "resid", "a2", "w2") if k in inp}
    K.gemm_set_variant(case["variant"])                                                            # 5.
    try:
        ws_bytes = K.lib().pso_conv2d_ws_bytes(B, Ho, Wo, Cout, K1, K2)
        assert (ws_bytes > 0) == case["ws"], f"{case_id}: workspace {ws_bytes} bytes"              # 6.
        got = K.conv2d(inp["x"], inp["w"], mode=mode, stride=stride, pad=pad, out_hw=(Ho, Wo), alpha=inp["alpha"],
                       out=out, out_dtype=odt, accumulate=case["mode"] == "acc", **kw)             # 7.
        name = K.lib().pso_last_kernel().decode()                                                  # 8.
    finally:
        K.gemm_set_variant(0)
    torch.cuda.synchronize()                                                                       # 9.
    assert got.data_ptr() == out.data_ptr()
    assert name.startswith(case["kernel"]), f"{case_id}: ran {name}, wanted {case['kernel']}"      # 10.
    check(f"conv {case_id}")                                                                       # 11.
    got2 = out.reshape(M, Cout).cpu()
    worst = ((got2.double() - ref).abs() / bound.clamp_min(_TINY)).max().item()
    print(f"\n[conv {K.ELEM} {case_id}] {name}: worst |err| / bound {worst:.3f} over {got2.numel()} elements",
          flush=True)                                                                              # 14. (before 12, 13)
    assert torch.isfinite(got2.float()).all(), f"{case_id}: a non-finite output (a tap read the NaN margin?)"   # 12.
    n, msg = violations(got2, ref, bound)                                                          # 13.
    assert n == 0, f"{case_id} ({name}): {msg}"
