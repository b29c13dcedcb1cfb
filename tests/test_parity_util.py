"""CPU self-test of tests/parity_util.py: the helper that the localised-error GPU parity tests stand on is itself
checked here, with no kernel involved -- the rounding model against fp64 on every attention shape the GPU tests use,
the guard-band detector, the reason the per-row metric exists, and the derived GEGLU / GEMM element-wise bounds against
a torch restatement of the documented computation (zero violations)."""
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
