"""The GEGLU epilogues and one small ragged case per GEMM dispatch family, with the outputs in guard-banded column
slices (parity_util.guarded: 8-element gaps either side, 64 guard rows, compared bit for bit) and an ELEMENT-WISE bound
against fp64 that is derived from the number formats (parity_util.geglu_reference / gemm_reference), in place of a
whole-tensor ratio: one wrong element fails, and so does one element written beside the output.
tests/test_parity_util.py checks on the CPU that a torch restatement of the documented computation violates these
bounds at zero elements on the same inputs; the kernels must do as well."""
import pytest
import torch

import parity_util as P

pytestmark = pytest.mark.gpu


@pytest.mark.knobs
@pytest.mark.parametrize("variant", [0, 31, 45, 57])  # the forms the GEGLU tests of test_gpu_kernels.py pin
@pytest.mark.parametrize("M,Fd,K,pre_rows", P.GEGLU_CASES)
def test_gemm_geglu_guarded_elementwise(cuda, variant, M, Fd, K, pre_rows):
    """gemm_geglu with out_pre / pre_rows and gemm_geglu_bwd: out, out_pre and the backward's out are row-strided column
    slices of guarded buffers; every element within the derived bound of the fp64 reference."""
    from pairwise_sample_optimization_amd import kernels as K_
    from pairwise_sample_optimization_amd._lib import PsoLibError
    inp = P.geglu_inputs(M, Fd, K, cuda)
    ref = P.geglu_reference(inp, Fd)
    idx = ref["idx"]
    wi, bi = inp["wp"][idx].contiguous(), inp["bp"][idx].contiguous()
    pr = pre_rows or M
    (out, din), check_a = P.guarded(M, [Fd, 2 * Fd], device=cuda)
    (pre,), check_b = P.guarded(pr, [2 * Fd], device=cuda)
    fwd_ok = (2 * Fd) % 256 == 0  # pso_gemm_geglu takes whole 256-column tiles of [h 32 | gate 32] groups only
    K_.gemm_set_variant(variant)
    try:
        if fwd_ok:
            assert K_.gemm_geglu(inp["x"], wi, bi, out_pre=pre, out=out, pre_rows=pre_rows).data_ptr() == out.data_ptr()
            fwd_kernel = K_.lib().pso_last_kernel().decode()
        else:  # refused as an argument error, nothing launched, nothing written
            with pytest.raises(PsoLibError, match="N % 256 == 0"):
                K_.gemm_geglu(inp["x"], wi, bi, out_pre=pre, out=out, pre_rows=pre_rows)
            fwd_kernel = "(refused: 2 * Fd is no multiple of 256)"
        assert K_.gemm_geglu_bwd(inp["dy"], inp["wo"], ref["pre_in"], out=din).data_ptr() == din.data_ptr()
        bwd_kernel = K_.lib().pso_last_kernel().decode()
    finally:
        K_.gemm_set_variant(0)
    torch.cuda.synchronize()
    print(f"\n[geglu {(M, Fd, K, pre_rows)} variant {variant}] fwd {fwd_kernel}; bwd {bwd_kernel}", flush=True)
    check_a(f"geglu {(M, Fd, K)} out | din")
    check_b(f"geglu {(M, Fd, K)} out_pre ({pr} rows)")
    if not fwd_ok:  # the forward's two views are gaps of their buffers now: still the fill, bit for bit
        for v in (out, pre):
            assert bool((v.view(torch.int16) == P.FILL_BITS[2]).all())
    fwd = [("out", out, ref["out"], ref["out_bound"]), ("out_pre", pre, ref["pre"][:pr], ref["pre_bound"][:pr])]
    for name, got, r, b in (fwd if fwd_ok else []) + [("din", din, ref["din"], ref["din_bound"])]:
        n, msg = P.violations(got, r, b)
        assert n == 0, f"{name}: {msg}"


@pytest.mark.knobs
@pytest.mark.parametrize("variant,case", [(c[0], k) for k, c in P.GEMM_CASES.items()])
def test_gemm_family_guarded_elementwise(cuda, variant, case):
    """One small ragged case per dispatch family of pso_gemm (2-phase, 8-phase 256 x 256 / 256 x 160 / 256 x 320,
    skinny-N, split-K workspace, the LoRA-tail forms with tail_group_n and tail_rows), bf16 output and fp32 accumulate,
    out= a column slice of a guarded buffer.  The kernel name is asserted so that a case cannot drift to another
    family; the families a small shape only reaches through a knob run in the tools-build child."""
    from pairwise_sample_optimization_amd import kernels as K_
    _, M, N, K, K2, group, tail_rows, mode, kernel = P.GEMM_CASES[case]
    inp = P.gemm_inputs(M, N, K, K2, group, tail_rows, mode, cuda)
    ref, bound = P.gemm_reference(inp, group, tail_rows, mode)
    (out,), check = P.guarded(M, [N], dtype=torch.float32 if mode == "acc" else K_.ELEM, device=cuda)
    kw = {k: inp[k] for k in ("bias", "resid", "a2", "w2") if k in inp}
    if mode == "acc":
        out.copy_(inp["base"])
        kw.update(out_dtype=torch.float32, accumulate=True)
    K_.gemm_set_variant(variant)
    try:
        if case.startswith("splitk-ws"):
            assert K_.lib().pso_gemm_ws_bytes(M, N, K, K2) > 0  # the shape takes the workspace split
        else:
            assert K_.lib().pso_gemm_ws_bytes(M, N, K, K2) == 0
        K_.gemm(inp["a"], inp["w"], alpha=inp["alpha"], out=out, tail_group_n=group, tail_rows=tail_rows, **kw)
        name = K_.lib().pso_last_kernel().decode()
    finally:
        K_.gemm_set_variant(0)
    torch.cuda.synchronize()
    assert name.startswith(kernel), f"{case}: ran {name}, wanted {kernel}..."
    check(f"gemm {case} {(M, N, K, K2)}")
    n, msg = P.violations(out, ref, bound)
    assert n == 0, f"{case} ({name}): {msg}"
