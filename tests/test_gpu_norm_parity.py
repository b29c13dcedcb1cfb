"""GroupNorm and LayerNorm (norm.hip) and the ordered LayerNorm parameter gradients (pso_layer_norm_dparam_ws), held
to localised bounds: the saved fp32 statistics against a derived bound, y and dx per 16-byte store chunk against 3 x
the rounding model, dgamma / dbeta element-wise, every output in a guard-banded buffer, every input ending where
payload NaNs begin.  All bounds come from the fp64 reference and the torch restatement of norm.hip's documented
roundings on the case's own inputs (tests/parity_util.py; NORM_F / NORM_F2 are derived in tests/test_parity_util.py
from a restatement with the kernels' chain lengths), never from a kernel's output.

The inputs are edge-weighted (parity_util.norm_inputs): pixel rows 0, 63, 64, HW - 1 (and 511, 512 under the 512-row
forward), LayerNorm channels 0 and C - 1 carry 32 x the weight of the rest in x and dy, so a dropped, doubled or
misattributed edge row moves its group's statistics by ~10^6 units of the bound and dx by tens of percent per chunk.

What each case is for is written beside it in parity_util.GN_CASES / GN_DPARAM_CASES / LN_CASES / LN_DPARAM_CASES."""
import pytest

import parity_util as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("B,HW,C,G", P.GN_CASES)
def test_group_norm_fwd_bwd(cuda, B, HW, C, G, silu):
    """Forward and backward with dadd, dgamma and dbeta at every block size gn_block gives (264, 480 and 512 threads
    included), Cg = 1 and Cg = C, the C limits, and either side of the forward's switch to 512-row blocks."""
    P.run_group_norm_case(cuda, B, HW, C, G, silu)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,HW", P.GN_DPARAM_CASES)
def test_group_norm_dparam_reduction_regimes(cuda, B, HW, accumulate):
    """B * HW / 64 = 1, 3 (single pass), 4, 5, 63 (split, ragged) and 64 (32 splits) row blocks at C = 64, over
    non-zero previous contents that must be added (accumulate) or must not show."""
    P.run_group_norm_case(cuda, B, HW, 64, 32, True, accumulate=accumulate)


@pytest.mark.parametrize("want", ["dgamma", "dbeta"])
def test_group_norm_one_dparam_only(cuda, want):
    """Only dgamma, only dbeta: the other pointer is null in the split reduction's final pass."""
    P.run_group_norm_case(cuda, 5, 64, 64, 32, True, accumulate=True, want=(want,))


@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_without_affine(cuda, silu):
    """gamma = beta = None: the null branches every GroupNorm kernel carries, forward and backward."""
    B, HW, C, G = P.GN_NOAFFINE_CASE
    P.run_group_norm_case(cuda, B, HW, C, G, silu, affine=False)


@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_shifted_input(cuda, silu):
    """x = 8 + 0.25 randn, mean / std ~ 32: var = E[x^2] - mean^2 cancels three digits, and the rstd bound's
    amplification term (E[x^2] + eps) / (var + eps) ~ 1000 is what admits a correct two-moment kernel and nothing
    looser."""
    B, HW, C, G = P.GN_SHIFTED_CASE
    P.run_group_norm_case(cuda, B, HW, C, G, silu, shifted=True)


@pytest.mark.parametrize("M,C", P.LN_CASES)
def test_layer_norm_fwd_bwd_strided(cuda, M, C):
    """Forward and backward the way unet.py calls them -- always with dadd -- on row-strided x, dy, dadd of three
    different leading dimensions, y and dx written into guarded column slices through out=."""
    P.run_layer_norm_case(cuda, M, C)


@pytest.mark.parametrize("M,C,strided", P.LN_DPARAM_CASES)
def test_layer_norm_dparam_ordered(cuda, M, C, strided):
    """K.layer_norm_dparam (the ordered product path): vector and scalar-tail loads, one- and two-level reductions,
    contiguous and strided rows; zero violations, and the same bits on a second call."""
    P.run_ln_dparam_case(cuda, M, C, strided)
