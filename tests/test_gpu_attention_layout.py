"""Attention as the UNet calls it: strided q / k / v slices in, outputs written straight into column slices of wider
buffers (unet.py: dq=d3[..., :C], dk=d3[..., C:2*C], dv=d3[..., 2*C:] for self-attention, dk=dk3[..., :C],
dv=dk3[..., C:] for cross-attention), checked per (batch, head, row) against fp64 and for stray stores.

Every output lives in a parity_util.guarded buffer -- 8-element gaps either side of each slice, 64 guard rows after the
last -- whose fill must survive bit for bit: a store one chunk too wide, a row stride taken for H*64, a tail predicate
that lets one row too many through all land in memory this test owns and looks at.  The comparison is
rowwise_rel(x, ref64, 64) over ALL heads, held to 3 x the worst row of parity_util.attention_model (the kernels'
documented roundings in plain torch) against the same fp64 reference: measured on the reference side, never on the
kernel (the factor's reasoning is at parity_util.ROW_BOUND_FACTOR).

What turns these tests red, read off attention.hip (mutants are reasoned about, not run: two of them store past the
end of a buffer):
  * an epilogue store one chunk too wide (attn_fwd2_kernel's `dt < 4` store loop run to 5): head H-1 writes columns
    C .. C+15 of its row, the gap after the slice -> check() of the forward's buffer names (row, column 8 + C) in every
    case; a fresh contiguous output would take it in the next row's head 0, which that row's owner overwrites.
  * `if (kr >= a.Sk) continue;` dropped in the dK/dV epilogue of attn_bwd_x_kernel or attn_bwd_dkv_kernel: in the
    unsplit cases (1, 1, 1, 5), (2, 2, 50, 77), (1, 2, 60, 130), (1, 2, 130, 300) the last batch's rows Sk .. are the
    guard rows -> check() of the dk | dv buffer reports "a guard row"; earlier batches' stray rows race with the next
    batch's first keys -> the per-row dk / dv assertion.
  * `a.lddk` replaced by `a.H * ATT_D` in a dK store (or `ldd` by `cols` in reduce_splits_kernel): equal for a
    contiguous output, which is all the older tests pass; here lddk is 2C + 24 or 3C + 32, so row kr lands kr * C
    elements on, across gaps and the dv slice -> check() fails and the unwritten dk rows keep the NaN fill ->
    the isfinite / per-row dk assertions (unsplit cases for the kernels' stores, split cases for the reduction)."""
import pytest

import parity_util as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,Sq,Sk", list(P.ATTN_CASES))
def test_attention_strided_in_guarded_out(cuda, B, H, Sq, Sk):
    """Forward (128 queries per workgroup: none of these shapes meets cdiv(Sq, 256) * H * B >= 1024) and backward in
    every regime of the backward's dispatch, smallest shapes that reach them (parity_util.ATTN_CASES says which)."""
    P.run_attention_case(cuda, B, H, Sq, Sk, P.ATTN_CASES[(B, H, Sq, Sk)])


def test_attention_fwd_256_queries_by_product_dispatch(cuda):
    """cdiv(300, 256) * 8 * 64 = 1024 >= 1024 and Sk = 130 > 128: pso_attention_fwd's own rule picks the
    256-queries-per-workgroup forward (attn_fwd2_kernel<4>), on a ragged second query block and a ragged third key
    tile.  Forward only."""
    B, H, Sq, Sk = P.ATTN_FWD256_CASE
    assert -(-Sq // 256) * H * B >= 1024 and Sk > 128
    P.run_attention_case(cuda, B, H, Sq, Sk, None, backward=False)


@pytest.mark.knobs
@pytest.mark.parametrize("variant", [0, 2, 4, 70])  # forward 32 / 64 rows per wave; 70: backward variant 7
@pytest.mark.parametrize("B,H,Sq,Sk", P.ATTN_RAGGED_CASES)
def test_attention_strided_in_guarded_out_forms(cuda, variant, B, H, Sq, Sk):
    """The two ragged cases under the forced forward tiles (variants 2 / 4) and under backward variant 7, which sends
    the short-key shape through the dQ + dK/dV launches (query-split there as well): same assertions."""
    from pairwise_sample_optimization_amd import kernels as K
    if variant:
        K.lib().pso_attention_set_variant(variant)
    try:
        P.run_attention_case(cuda, B, H, Sq, Sk, True)
    finally:
        if variant:
            K.lib().pso_attention_set_variant(0)
