"""CPU self-test of tests/parity_util.py: the helper that the localised-error GPU parity tests stand on is itself
checked here, with no kernel involved -- the rounding model against fp64 on every attention shape the GPU tests use,
the guard-band detector, the reason the per-row metric exists, and the derived GEGLU / GEMM / convolution element-wise
bounds against a torch restatement of the documented computation (zero violations), with planted faults that must land
outside them; the conv cases' dispatch is asked of the plan query, which launches nothing."""
import functools
import math

import pytest
import torch

import parity_util as P

SCALE = 64 ** -0.5
_SHAPES = list(P.ATTN_CASES) + [P.ATTN_FWD256_CASE]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_attention_model_against_fp64_on_every_named_shape(dtype):
    """attention_model against attention_fp64 on every shape of tests/test_gpu_attention_layout.py: finite, and a worst
    row of rounding size (printed: 3 x this is the bound the kernels are held to)."""
    for B, H, Sq, Sk in _SHAPES:
        fwd_only = (B, H, Sq, Sk) == P.ATTN_FWD256_CASE
        q, k, v, do = P.attention_inputs(B, H, Sq, Sk, dtype, "cpu")
        do = None if fwd_only else do
        model = P.attention_model(q, k, v, do, H, SCALE)
        ref = P.attention_fp64(q, k, v, do, H, SCALE)
        assert all(torch.isfinite(t.float()).all() for t in model)
        assert all(torch.isfinite(t).all() for t in ref)
        worst = P.attention_row_bounds(model, ref)
        print(f"{(B, H, Sq, Sk)} {dtype}: " + ", ".join(f"{n} {e}" for n, e in worst.items())
              + f", lse {(model[1].double() - ref[1]).abs().max().item():.2e}")
        one_ulp = 2.0 ** (-8 if dtype == torch.bfloat16 else -11)  # a whole ulp of the element type, relative
        for n, e in worst.items():
            # no row is exact, and none is worse than a few roundings of the element type (a modelling slip -- a
            # transposed head, a missing scale -- would be O(1))
            assert 0 < e < 4 * one_ulp, (n, e)
        assert (model[1].double() - ref[1]).abs().max().item() < 2e-3


def test_rowwise_rel_names_the_row():
    ref = torch.randn(2, 7, 3 * 64, dtype=torch.float64)
    got = ref.clone()
    got[1, 4, 64 + 8:64 + 12] = 0
    e = P.rowwise_rel(got, ref, 64)
    assert e.index == (1, 4, 1) and 0.05 < e < 1
    got[0, 2, 130] = float("nan")
    e = P.rowwise_rel(got, ref, 64)
    assert e != e and e.index == (0, 2, 2)  # NaN: fails every `<`
    assert not e < 1.0


def test_guarded_detects_only_outside_writes():
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        (a, b), check = P.guarded(37, [64, 100], dtype=dtype, device="cpu")
        assert a.shape == (37, 64) and b.shape == (37, 100) and a.stride(0) == b.stride(0)
        assert a.stride(0) % 8 == 0 and a.stride(1) == 1
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        assert torch.isnan(a).all()          # the fill reads as NaN: a kernel that loaded it would show it
        check()
        a.copy_(torch.randn(37, 64))         # writes inside the views are the kernel's business
        b.zero_()
        b[5, 99] = float("nan")
        check()
        base = a._base if a._base is not None else a
        ld = a.stride(0)
        for r, c in ((0, 7), (36, 8 + 64), (10, ld - 1), (37, 8), (37 + 63, 20)):  # gaps either side, guard rows
            old = base[r, c].clone()
            base[r, c] = 0.0
            with pytest.raises(AssertionError, match=rf"row {r}, column {c}\)"):
                check()
            base[r, c] = float("nan")        # a canonical NaN is not the fill either
            with pytest.raises(AssertionError, match=rf"row {r}, column {c}\)"):
                check()
            base.view(torch.int16 if dtype != torch.float32 else torch.int32)[r, c] = \
                old.view(torch.int16 if dtype != torch.float32 else torch.int32)
            check()


def test_one_chunk_error_is_invisible_to_the_whole_tensor_ratio():
    """Why the helper exists: zero one 4-element store chunk of one row of the model's output at (2, 5, 300, 77).  The
    whole-tensor ratio stays under the 1e-2 bar the older tests use; the per-row metric jumps far above the bound."""
    B, H, Sq, Sk = 2, 5, 300, 77
    q, k, v, _ = P.attention_inputs(B, H, Sq, Sk, torch.bfloat16, "cpu")
    o, _ = P.attention_model(q, k, v, None, H, SCALE)
    o64, _ = P.attention_fp64(q, k, v, None, H, SCALE)
    bound = P.ROW_BOUND_FACTOR * P.rowwise_rel(o, o64, 64)
    assert P.rowwise_rel(o, o64, 64) < bound < 2e-2
    bad = o.clone()
    bad[1, 299, 3 * 64 + 60:3 * 64 + 64] = 0   # the last chunk of head 3 in the last (ragged-tile) row
    assert P.frob_rel(bad, o64) < 1e-2          # today's metric: passes
    e = P.rowwise_rel(bad, o64, 64)
    assert e > bound and e > 0.05 and e.index == (1, 299, 3), e
    # one whole (batch, head, row) zeroed -- sqrt(1 / 3000) = 1.8e-2 of the tensor -- sits right at the older
    # dQ / dK / dV bar of 2e-2 at this shape: over or under it by the luck of that row's norm
    bad = o.clone()
    bad[0, 17, 64:128] = 0
    assert 1.5e-2 < P.frob_rel(bad, o64) < 3e-2 and P.rowwise_rel(bad, o64, 64) > 0.99


def test_qsplit_from_ws_bytes():
    d = -(-(2 * 5 * 300 * 4) // 256) * 256
    assert P.qsplit_from_ws_bytes(2 * d, 2, 5, 300, 77) == 1
    assert P.qsplit_from_ws_bytes(2 * d + 5 * 2 * 2 * 77 * 5 * 64 * 4, 2, 5, 300, 77) == 5


@pytest.mark.parametrize("M,Fd,K,pre_rows", P.GEGLU_CASES)
def test_geglu_bounds_hold_for_the_restatement(M, Fd, K, pre_rows):
    """The derived element-wise bounds are violated at ZERO elements by a torch restatement of the documented GEGLU
    computation (fp32 matmul, bf16 pre-activation, fp32 epilogue, bf16 output) on the GPU test's own inputs -- and by
    many elements once one pre-activation column is shifted by one."""
    inp = P.geglu_inputs(M, Fd, K, "cpu")
    ref = P.geglu_reference(inp, Fd)
    out, pre, din = P.geglu_restatement(inp, Fd, ref["pre_in"])
    for name, got in (("out", out), ("pre", pre), ("din", din)):
        n, msg = P.violations(got, ref[name], ref[name + "_bound"])
        assert n == 0, (name, msg)
    assert P.violations(torch.roll(out, 1, 1), ref["out"], ref["out_bound"])[0] > out.numel() // 2
    assert P.violations(torch.roll(din, 1, 1), ref["din"], ref["din_bound"])[0] > din.numel() // 2
    one = out.clone()
    one[M - 1, Fd - 4:] = 0
    assert 1 <= P.violations(one, ref["out"], ref["out_bound"])[0] <= 4


@pytest.mark.parametrize("case", list(P.GEMM_CASES))
def test_gemm_bound_holds_for_the_restatement(case):
    variant, M, N, K, K2, group, tail_rows, mode, _ = P.GEMM_CASES[case]
    inp = P.gemm_inputs(M, N, K, K2, group, tail_rows, mode, "cpu")
    ref, bound = P.gemm_reference(inp, group, tail_rows, mode)
    got = P.gemm_restatement(inp, group, tail_rows, mode)
    n, msg = P.violations(got, ref, bound)
    assert n == 0, msg
    assert P.violations(torch.roll(got, 1, 1), ref, bound)[0] > got.numel() // 2


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm helpers
# ----------------------------------------------------------------------------------------------------------------------
_DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def _gn_named():
    """Every GroupNorm configuration tests/test_gpu_norm_parity.py runs: (shape, silu, affine, shifted)."""
    for shape in P.GN_CASES:
        for silu in (False, True):
            yield shape, silu, True, False
    for silu in (False, True):
        yield P.GN_NOAFFINE_CASE, silu, False, False
        yield P.GN_SHIFTED_CASE, silu, True, True
    for B, HW in P.GN_DPARAM_CASES:
        yield (B, HW, 64, 32), True, True, False


def _gn_case(shape, silu, affine, shifted, dtype):
    inp = P.norm_inputs("gn", shape, dtype, "cpu", shifted)
    gamma, beta = (inp["gamma"], inp["beta"]) if affine else (None, None)
    return inp, gamma, beta, P.gn_reference(inp["x"], gamma, beta, shape[3], P.NORM_EPS, silu, inp["dy"], inp["dadd"])


@functools.lru_cache(maxsize=None)
def _ln_case(M, C, dtype):
    inp = P.norm_inputs("ln", (M, C), dtype, "cpu")
    return inp, P.ln_reference(inp["x"], inp["gamma"], inp["beta"], P.NORM_EPS, inp["dy"], inp["dadd"])


def _check_model(tag, model, ref, dtype, f2=None):
    """The four points every named case must meet: finite, worst chunk of rounding size, statistics inside the derived
    bound, no parameter gradient outside its own."""
    y, stats, dx, dgamma, dbeta = model
    assert all(torch.isfinite(t.float()).all() for t in model), tag
    assert all(torch.isfinite(ref[n]).all() for n in ("y", "stats", "dx", "dgamma", "dbeta")), tag
    worst = P.norm_chunk_bounds(model, ref)
    mu, ru = P.norm_stats_units(stats, ref)
    ug = P.norm_dparam_units({"dgamma": dgamma, "dbeta": dbeta}, ref, {})
    print(f"{tag}: y {worst['y']}, dx {worst['dx']}, stats units {mu:.2f} {ru:.2f}, dparam units {ug}")
    for n, e in worst.items():
        assert 0 < e < 4 * P.ELEM_ULP[dtype], (tag, n, e)
    assert mu <= P.NORM_F and ru <= P.NORM_F, (tag, mu, ru)
    bg, bb = P.norm_dparam_bounds(ref, {}, f2)
    assert P.violations(dgamma.reshape(1, -1), ref["dgamma"].reshape(1, -1), bg.reshape(1, -1))[0] == 0, tag
    assert P.violations(dbeta.reshape(1, -1), ref["dbeta"].reshape(1, -1), bb.reshape(1, -1))[0] == 0, tag


@_DTYPES
def test_group_norm_model_against_fp64_on_every_named_case(dtype):
    for shape, silu, affine, shifted in _gn_named():
        inp, gamma, beta, ref = _gn_case(shape, silu, affine, shifted, dtype)
        model = P.group_norm_model(inp["x"], gamma, beta, shape[3], P.NORM_EPS, silu, inp["dy"], inp["dadd"])
        _check_model(f"gn {shape} silu={silu} affine={affine} shifted={shifted} {dtype}", model, ref, dtype,
                     P.NORM_F2 if shifted else None)
        for got, want in zip(P.group_norm_fp64(inp["x"], gamma, beta, shape[3], P.NORM_EPS, silu, inp["dy"],
                                               inp["dadd"]), ("y", "stats", "dx", "dgamma", "dbeta")):
            assert got.dtype == torch.float64 and torch.equal(got, ref[want])


@_DTYPES
def test_layer_norm_model_against_fp64_on_every_named_case(dtype):
    for M, C in P.LN_CASES + [(m, c) for m, c, _ in P.LN_DPARAM_CASES]:
        inp, ref = _ln_case(M, C, dtype)
        if C % 8:   # the dparam-only shapes with a scalar tail: no 8-chunks to compare, the sums only
            st, _, dg, db = P.layer_norm_model(inp["x"], inp["gamma"], inp["beta"], P.NORM_EPS, inp["dy"],
                                               inp["dadd"])[1:]
            ref = P.ln_dparam_reference(inp["x"], inp["dy"], st)
            bg, bb = P.norm_dparam_bounds(ref, {})
            assert P.violations(dg.reshape(1, -1), ref["dgamma"].reshape(1, -1), bg.reshape(1, -1))[0] == 0
            assert P.violations(db.reshape(1, -1), ref["dbeta"].reshape(1, -1), bb.reshape(1, -1))[0] == 0
            continue
        model = P.layer_norm_model(inp["x"], inp["gamma"], inp["beta"], P.NORM_EPS, inp["dy"], inp["dadd"])
        # the parameter gradients are an op of their own, whose inputs include the statistics: the model's here
        ref = dict(ref, **P.ln_dparam_reference(inp["x"], inp["dy"], model[1]))
        _check_model(f"ln {(M, C)} {dtype}", model, ref, dtype)


def _f_from(worst):
    """Four times the worst measured ratio, rounded up to a power of two, no smaller than 8."""
    return max(8.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))


def test_norm_F_and_F2_come_from_the_kernel_order_restatement():
    """NORM_F and NORM_F2 are derived here, not from a kernel run: every fp32 sum of every named case is restated with
    the kernels' own sequential chain lengths (parity_util.*_kernel_order), in bf16 and fp16; the worst error in units
    of the bound expressions is printed, and each constant must be 4 x its worst, rounded up to a power of two and no
    smaller than 8."""
    w_mean = w_rstd = w_dp = w_dpc = 0.0
    gen = torch.Generator().manual_seed(5)
    for dtype in (torch.bfloat16, torch.float16):
        for shape, silu, affine, shifted in _gn_named():
            inp, gamma, beta, ref = _gn_case(shape, silu, affine, shifted, dtype)
            stats, dg, db = P.gn_kernel_order(inp["x"], gamma, beta, shape[3], P.NORM_EPS, silu, inp["dy"])
            mu, ru = P.norm_stats_units(stats, ref)
            ug = P.norm_dparam_units({"dgamma": dg, "dbeta": db}, ref, {})
            w_mean, w_rstd = max(w_mean, mu), max(w_rstd, ru)
            # accumulate=True: one more fp32 add onto the previous contents, with its own allowance
            prev = {n: torch.randn(shape[2], generator=gen) for n in ("dgamma", "dbeta")}
            ua = P.norm_dparam_units({"dgamma": prev["dgamma"] + dg, "dbeta": prev["dbeta"] + db}, ref, prev)
            w_dp = max(w_dp, *ug.values(), *ua.values())
            if not shifted:
                w_dpc = max(w_dpc, *ug.values(), *ua.values())
        for M, C in P.LN_CASES:
            inp, ref = _ln_case(M, C, dtype)
            mu, ru = P.norm_stats_units(P.ln_stats_kernel_order(inp["x"], P.NORM_EPS), ref)
            w_mean, w_rstd = max(w_mean, mu), max(w_rstd, ru)
        for M, C, _ in P.LN_DPARAM_CASES:
            inp, ref = _ln_case(M, C, dtype)
            prev = {n: torch.randn(C, generator=gen) for n in ("dgamma", "dbeta")}
            stats = ref["stats"].float()
            dg, db = P.ln_dparam_kernel_order(inp["x"], inp["dy"], stats, prev["dgamma"], prev["dbeta"])
            ug = P.norm_dparam_units({"dgamma": dg, "dbeta": db}, P.ln_dparam_reference(inp["x"], inp["dy"], stats), prev)
            w_dp, w_dpc = max(w_dp, *ug.values()), max(w_dpc, *ug.values())
    print(f"\nkernel-order restatement, worst over every named case: mean {w_mean:.3f} units, rstd {w_rstd:.3f} units "
          f"-> F = {_f_from(max(w_mean, w_rstd)):g}; dgamma / dbeta {w_dp:.3f} units -> F2 = {_f_from(w_dp):g}; "
          f"without the shifted case {w_dpc:.3f} units -> F2 (centred) = {_f_from(w_dpc):g}")
    assert 0 < w_mean and 0 < w_rstd and 0 < w_dpc <= w_dp
    assert P.NORM_F == _f_from(max(w_mean, w_rstd)), (P.NORM_F, w_mean, w_rstd)
    assert P.NORM_F2 == _f_from(w_dp), (P.NORM_F2, w_dp)
    assert P.NORM_F2_CENTRED == _f_from(w_dpc), (P.NORM_F2_CENTRED, w_dpc)


def test_ln_dparam_plan_reaches_the_named_regimes():
    assert P.ln_dparam_plan(1) == (1, 1, 1) and P.ln_dparam_plan(65) == (2, 2, 1)
    assert P.ln_dparam_plan(48 * 64) == (48, 48, 1)
    assert P.ln_dparam_plan(3100) == (49, 2, 25)     # two levels, splits of 25 and 24 row blocks
    assert P.ln_dparam_plan(4200) == (66, 3, 22)
    assert [P.gn_slots(c) for c in (8, 32, 64, 128, 264, 320, 960, 1920, 4096)] == [512, 128, 64, 32, 8, 8, 4, 2, 1]
    assert [(c // 8) * P.gn_slots(c) for c in (264, 960, 1920)] == [264, 480, 480]
    assert P.gn_rows_fwd(16384) == 64 and P.gn_rows_fwd(16385) == 512
    assert P.gn_edge_rows(100) == [0, 63, 64, 99] and P.gn_edge_rows(64) == [0, 63]
    assert P.gn_edge_rows(16500) == [0, 63, 64, 511, 512, 16499]


@_DTYPES
def test_norm_detectors_wrong_statistics_land_outside_the_bound(dtype):
    """Deliberately wrong restatements of the statistics, each far outside the bound a correct one meets: the last
    pixel row left out, row 64 counted twice, the LayerNorm mean over C - 8 channels -- and, for contrast, the
    whole-tensor ratio of the y they give, which the older 8e-3 bar lets through."""
    B, HW, C, G = shape = (2, 100, 320, 32)
    inp, gamma, beta, ref = _gn_case(shape, False, True, False, dtype)
    x = inp["x"]
    n = float(HW * (C // G))
    good = P.group_norm_model(x, gamma, beta, G, P.NORM_EPS, False)
    assert max(P.norm_stats_units(good[1], ref)) <= P.NORM_F
    xf = x.float()

    def sums(v):
        return P.gn_group_combine(P.gn_chunk_sums(v, 64), G)

    # (a) every block stops one row early: the image's last row never enters the sums (the divisor stays HW * Cg)
    a, q = sums(xf[:, :HW - 1]), sums(xf[:, :HW - 1] ** 2)
    lost = P.gn_stats_from_sums(a, q, n, P.NORM_EPS)
    # (b) the row at the block boundary is taken by both blocks
    a, q = sums(xf) + sums(xf[:, 64:65]), sums(xf * xf) + sums(xf[:, 64:65] ** 2)
    twice = P.gn_stats_from_sums(a, q, n, P.NORM_EPS)
    for name, bad in (("last row lost", lost), ("row 64 twice", twice)):
        mu, ru = P.norm_stats_units(bad, ref)
        print(f"{name} {dtype}: stats units mean {mu:.0f} rstd {ru:.0f} (bound {P.NORM_F:g})")
        assert ru > 1000 * P.NORM_F / 8, (name, mu, ru)
    # an unweighted row shows what the Frobenius bar cannot see: rstd off by percents of a percent, y inside 8e-3
    plain = torch.randn(1, 100, 64).to(dtype)
    pref = P.gn_reference(plain, None, None, 2, P.NORM_EPS, False)
    pf = plain.float()
    a = P.gn_group_combine(P.gn_chunk_sums(pf[:, :99], 64), 2)
    q = P.gn_group_combine(P.gn_chunk_sums(pf[:, :99] ** 2, 64), 2)
    bad = P.gn_stats_from_sums(a, q, 100.0 * 32, P.NORM_EPS)
    ybad = P.group_norm_model(plain, None, None, 2, P.NORM_EPS, False, stats=bad)[0]
    assert P.frob_rel(ybad, pref["y"]) < 8e-3 and P.norm_stats_units(bad, pref)[1] > 100 * P.NORM_F
    # (c) LayerNorm statistics over C - 8 channels (a lane's last chunk masked off)
    M, C = 7, 520
    inp, ref = _ln_case(M, C, dtype)
    good = P.layer_norm_model(inp["x"], inp["gamma"], inp["beta"], P.NORM_EPS)
    assert max(P.norm_stats_units(good[1], ref)) <= P.NORM_F
    xs = inp["x"].float()[:, :C - 8]
    mean = xs.sum(1, keepdim=True) / C
    bad = torch.cat([mean, torch.rsqrt(((xs - mean) ** 2).sum(1, keepdim=True) / C + P.NORM_EPS)], 1)
    mu, ru = P.norm_stats_units(bad, ref)
    print(f"LN mean over C - 8 {dtype}: stats units mean {mu:.0f} rstd {ru:.0f}")
    assert mu > 1000 * P.NORM_F / 8 and ru > 1000 * P.NORM_F / 8


@_DTYPES
def test_norm_detector_neighbours_coefficients_land_outside_the_chunk_bound(dtype):
    """dx with every group's backward coefficients taken from its neighbour (g -> g + 1): the whole-tensor ratio may
    stay small, the worst 8-chunk leaves 3 x the model's by more than an order of magnitude."""
    B, HW, C, G = shape = (2, 100, 320, 32)
    inp, gamma, beta, ref = _gn_case(shape, True, True, False, dtype)
    args = (inp["x"], gamma, beta, G, P.NORM_EPS, True, inp["dy"], inp["dadd"])
    model = P.group_norm_model(*args)
    bound = P.ROW_BOUND_FACTOR * P.norm_chunk_bounds(model, ref)["dx"]
    coef, _, _ = P.gn_model_coef(inp["x"], inp["dy"], model[1], gamma, beta, G, True)
    bad = P.group_norm_model(*args, coef=torch.roll(coef, 1, 1))
    e = P.rowwise_rel(bad[2], ref["dx"], 8)
    print(f"neighbour's coefficients {dtype}: worst dx chunk {e}, bound {bound:.3e}")
    assert P.rowwise_rel(model[2], ref["dx"], 8) < bound < e and e > 0.1
    # and one group only (group 5 of image 1 uses group 6's): found, and named
    one = coef.clone()
    one[1, 5] = coef[1, 6]
    e = P.rowwise_rel(P.group_norm_model(*args, coef=one)[2], ref["dx"], 8)
    assert e > bound and e.index[0] == 1 and e.index[2] in (50 // 8, 59 // 8, 6, 7), e


# ----------------------------------------------------------------------------------------------------------------------
# convolutions
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(case_id, dtype):
    """(inputs, fp64 reference, bound) of one conv case, computed once and shared (read-only) by the tests below."""
    case = P.CONV_CASES[case_id]
    inp = P.conv_inputs(case, dtype, "cpu")
    return (inp,) + P.conv_reference(inp, case)


def test_conv_case_table_is_the_issued_one():
    """The ids, split between the product dispatch and the knob-pinned forms, and the facts the cases are about: two
    images in one 64-row tile with a ragged last tile, non-square images everywhere but the 8-phase one-tile cases,
    the asymmetric downsample's last tap past the bottom and right edge."""
    assert len(P.CONV_DEFAULT_IDS) == 19 and len(P.CONV_KNOB_IDS) == 10
    for cid, c in P.CONV_CASES.items():
        _, _, _, Ho, Wo = P.conv_geom(c)
        assert c["B"] * Ho * Wo <= (1024 if c["Cout"] <= 3 else 768), cid   # small on purpose
        assert c["H"] != c["W"] or cid in ("8p-one-tile", "8p-three-images"), cid
    c = P.CONV_CASES["s1-straddle"]
    assert (c["H"] * c["W"], c["B"] * c["H"] * c["W"]) == (63, 189) and c["Cout"] % 64
    c = P.CONV_CASES["s2asym-vae"]
    assert P.conv_geom(c)[1:] == (2, 0, 5, 3) and 2 * (5 - 1) + 2 == c["H"] and 2 * (3 - 1) + 2 == c["W"]
    assert P.conv_geom(P.CONV_CASES["s2-odd"])[3:] == (5, 4) and P.conv_geom(P.CONV_CASES["s2-even"])[3:] == (4, 3)
    inp = P.conv_inputs(P.CONV_CASES["s1-concat"], torch.bfloat16, "cpu")
    for n in ("x", "x2"):   # the images end where the NaN begins, at least (W + 2) * C elements of it either side
        t = inp[n]
        base, off, C = t._base, t.storage_offset(), t.shape[3]
        assert off >= (t.shape[2] + 2) * C and base.numel() - off - t.numel() >= (t.shape[2] + 2) * C
        assert torch.isnan(base[:off]).all() and torch.isnan(base[off + t.numel():]).all() and torch.isfinite(t).all()
        assert off % 8 == 0 and t.is_contiguous()


@_DTYPES
def test_conv_bound_holds_for_the_restatement(dtype):
    """conv_restatement (the documented gather and roundings, in fp32 torch) against conv_reference (fp64, torch's own
    conv operators) on every case id: zero violations of the derived bound.  It also ties the two descriptions of each
    gather mode to one another.  The worst ratios are recorded beside P.CONV_CASES."""
    worst = {}
    for cid, case in P.CONV_CASES.items():
        inp, ref, bound = _conv_case(cid, dtype)
        got = P.conv_restatement(inp, case)
        assert got.dtype == (torch.float32 if case["mode"] in ("f32", "acc") else dtype)
        n, msg = P.violations(got, ref, bound)
        worst[cid] = ((got.double() - ref).abs() / bound).max().item()
        print(f"conv {cid} {dtype}: worst |err| / bound {worst[cid]:.3f} over {got.numel()} elements")
        assert n == 0, (cid, msg)
        assert P.violations(torch.roll(got, 1, 0), ref, bound)[0] > got.numel() // 2, cid   # the next pixel's row
    print(f"conv {dtype}: worst over all ids {max(worst.values()):.3f} ({max(worst, key=worst.get)})")
    assert 0.3 < max(worst.values()) <= 1.0   # a 16-bit rounding uses a good part of its unit roundoff


_CONV_DETECTORS = [("wrap", "s1-straddle"), ("replicate", "up2"), ("pad-top-left", "s2asym-vae"),
                   ("rowbias-tile", "s1-straddle"), ("t2-swap", "t2-even"), ("epilogue-per-split", "splitk")]


@_DTYPES
@pytest.mark.parametrize("fault,case_id", _CONV_DETECTORS)
def test_conv_detectors_planted_faults_land_outside_the_bound(fault, case_id, dtype):
    """Each planted fault of the restatement gives at least one violation; the whole-tensor ratio is printed beside."""
    case = P.CONV_CASES[case_id]
    inp, ref, bound = _conv_case(case_id, dtype)
    bad = P.conv_restatement(inp, case, fault)
    n, msg = P.violations(bad, ref, bound)
    print(f"conv detector {fault} on {case_id} {dtype}: {n} of {bad.numel()} elements outside the bound, whole-tensor "
          f"ratio {P.frob_rel(bad, ref):.3e}")
    assert n >= 1, (fault, case_id)
    if fault == "rowbias-tile":   # rows 126, 127: the two pixels of image 2 inside the tile that starts in image 1
        err = (bad.double() - ref).abs() > bound
        assert set(err.any(1).nonzero().reshape(-1).tolist()) == {126, 127}


@_DTYPES
def test_conv_wrapped_tap_is_invisible_to_the_whole_tensor_ratio(dtype):
    """The first detector against the metric of the older conv tests.  With the horizontal bound missing at every
    left / right edge pixel of this 9 x 7 image the whole-tensor ratio is large too (2 of 7 pixel columns are wrong);
    what that ratio cannot see is the mistake one lane makes: one 16-byte chunk of the left tap of ONE edge pixel
    taken from the neighbouring row.  Planted at each left-edge pixel of the last image in turn: the element-wise bound
    finds every one of them and names the pixel; the 4e-3 ratio the older tests assert lets some of them pass (measured:
    3 of 8 in bf16, 5 of 8 in fp16, the others reach at most 6e-3 -- and on the older tests' own, larger shapes one
    pixel is a far smaller share of the tensor than 1 / 189 here)."""
    case = P.CONV_CASES["s1-straddle"]
    inp, ref, bound = _conv_case("s1-straddle", dtype)
    assert P.frob_rel(P.conv_restatement(inp, case), ref) < 4e-3
    assert P.frob_rel(P.conv_restatement(inp, case, "wrap"), ref) > 4e-3
    passed = []
    for oy in range(1, case["H"]):   # row 0 has no neighbouring row above inside the image
        bad = P.conv_restatement(inp, case, "wrap-one-chunk", at=oy)
        n, _ = P.violations(bad, ref, bound)
        fr = P.frob_rel(bad, ref)
        rows = ((bad.double() - ref).abs() > bound).any(1).nonzero().reshape(-1).tolist()
        print(f"one wrapped chunk at row {oy} {dtype}: {n} elements outside the bound, whole-tensor ratio {fr:.3e}")
        assert n >= 1 and rows == [2 * 63 + oy * 7], (oy, n, rows)
        passed.append(fr < 4e-3)
    assert any(passed), passed


def test_guarded_flat_detects_only_outside_writes():
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        view, check = P.guarded_flat(1000, dtype=dtype, device="cpu", pad=64)
        assert view.shape == (1000,) and view.is_contiguous() and view.data_ptr() % 16 == 0
        assert torch.isnan(view).all()
        check()
        view.copy_(torch.randn(1000))   # a write inside the view is the kernel's business
        view[999] = float("nan")
        check()
        base = view._base
        for i in (0, 63, 64 + 1000, 64 + 1000 + 63):   # before the view, and after it
            base[i] = 0.0
            with pytest.raises(AssertionError, match=rf"first at {i} of"):
                check()
            base[i] = float("nan")          # a canonical NaN is not the fill either
            with pytest.raises(AssertionError, match=rf"first at {i} of"):
                check()
            base.view(torch.int32 if dtype == torch.float32 else torch.int16)[i] = P.FILL_BITS[view.element_size()]
            check()


_CONV_PLAN_PROBE = """
import ctypes, json, sys
sys.path.insert(0, "tests")
import gemm_plan_cases as C
import parity_util as P
from pairwise_sample_optimization_amd import _lib
l = _lib.lib()
got = {}
for cid in P.CONV_CASES:
    case = P.conv_plan_case(cid)
    q, info = _lib.PsoGemmPlanQuery(**C.full(case)), _lib.PsoGemmPlanInfo()
    rc = l.pso_gemm_plan_query(C.PLAN_CONV, ctypes.byref(q), ctypes.byref(info))
    got[cid] = C.plan_of_info(C.PLAN_CONV, info) if rc == 0 else ["error", rc, l.pso_last_error().decode()]
json.dump(got, sys.stdout)
"""


def test_conv_cases_plan_their_named_forms():
    """Every conv case id, with the operand alignments and row pitches run_conv_case hands over, plans the form its
    kernel name says (csrc/gemm_plan.h through pso_gemm_plan_query, which launches nothing; a PSO_LIB=knobs child as in
    tests/test_gemm_plan_cpu.py): the tile, the conv mode (1 NORMAL, 2 UP2, 3 T2), the workspace K-splits, the 8-phase
    conv form, the direct small-Cout kernel -- and the strided-output Cout = 3 case NOT the direct kernel."""
    import json
    import os
    import subprocess
    import sys
    import gemm_plan_cases as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "PSO_LIB_PATH"}
    env["PSO_LIB"] = "knobs"
    r = subprocess.run([sys.executable, "-c", _CONV_PLAN_PROBE], env=env, cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout)
    assert set(got) == set(P.CONV_CASES)
    wrong = {cid: (got[cid], C.plan_of_kernel(c["kernel"], c["ws_ks"])) for cid, c in P.CONV_CASES.items()
             if got[cid] != C.plan_of_kernel(c["kernel"], c["ws_ks"])}
    assert not wrong, f"(planned, named): {wrong}"
    modes = {cid: got[cid][7] for cid, c in P.CONV_CASES.items() if got[cid][0] == "tile"}
    assert modes["up2"] == P.CONV_UP2 and modes["t2-odd"] == modes["t2-even"] == P.CONV_T2
    assert modes["small-strided-out"] == P.CONV_NORMAL and got["small-c3"][0] == "small_conv"
    assert got["splitk"][9] == got["splitk-concat"][9] == 2 and got["splitk-off"][9] == 0
