"""Every convolution path -- the 2-phase implicit GEMM's three gather modes (gemm.hip issue_tile), its register-
pipelined gather (load_chunk_conv), the 8-phase 256 x 320 conv form (gemm8p.hip CONV), the workspace split-K and the
direct small-Cout kernel (conv_small.hip) -- at small non-square shapes where two images share a 64-row tile and the last
tile is ragged, each held ELEMENT-WISE to an fp64 reference built from torch's own conv operators
(parity_util.conv_reference): inputs inside NaN margins, the output a guard-banded column slice (ldo > Cout) whose
surroundings must keep their fill bit for bit, the launched kernel asserted by name, zero elements outside the bound
derived from the number formats.  tests/test_parity_util.py checks on the CPU that a torch restatement of the documented
computation meets these bounds at every case, that planted border / tile / split faults do not, and that every case
plans its named form."""
import pytest
import torch

import parity_util as P

pytestmark = pytest.mark.gpu


@pytest.mark.knob_variants
@pytest.mark.parametrize("case", P.CONV_DEFAULT_IDS)
def test_conv_guarded_elementwise(cuda, case):
    """The forms the automatic dispatch takes at these shapes, in the product library and (knob_variants: it runs in
    the tools-build child too) in the tools build alike."""
    P.run_conv_case(cuda, case)


@pytest.mark.knobs
@pytest.mark.parametrize("variant,case", [(P.CONV_CASES[k]["variant"], k) for k in P.CONV_KNOB_IDS])
def test_conv_guarded_elementwise_pinned_forms(cuda, variant, case):
    """The forms a small shape only reaches through a knob (the 8-phase conv tiles, the UNet's 2-phase tile shapes, the
    register-pipelined gather, the workspace split switched off): these run in the tools-build child."""
    assert variant == P.CONV_CASES[case]["variant"] != 0
    P.run_conv_case(cuda, case)


def _conv_operands(cuda, B=2, H=9, W=7, C=64, Cout=64):
    from pairwise_sample_optimization_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g).to(K.ELEM).to(cuda)
    w = (torch.randn(Cout, 3, 3, C, generator=g) / (3 * C ** 0.5)).to(K.ELEM).to(cuda)
    return K, x, w


def test_conv_out_layout_that_is_no_row_pitch_raises(cuda):
    """kernels.conv2d takes out= (and resid=) as [B * Ho * Wo, ld >= Cout] rows; any other strided layout -- here a
    transposed one -- raises ValueError before anything is launched, instead of being written as if it were dense."""
    K, x, w = _conv_operands(cuda)
    B, H, W, Cout = 2, 9, 7, 64
    fill = torch.full((B, W, H, Cout), 7.0, dtype=K.ELEM, device=cuda)
    before = K.lib().pso_last_kernel().decode()   # the note of whatever ran last: no launch may replace it
    with pytest.raises(ValueError, match="row-pitched"):
        K.conv2d(x, w, out=fill.transpose(1, 2))
    with pytest.raises(ValueError, match="shape"):
        K.conv2d(x, w, out=fill)   # [B, W, H, Cout]: the wrong shape
    good = torch.empty(B, H, W, Cout, dtype=K.ELEM, device=cuda)
    with pytest.raises(ValueError, match="resid"):
        K.conv2d(x, w, resid=fill.transpose(1, 2), out=good)
    torch.cuda.synchronize()
    assert K.lib().pso_last_kernel().decode() == before and bool((fill == 7.0).all())


def test_conv_resid_row_pitch_is_honoured(cuda):
    """resid= as a column slice of a wider buffer (ldr > Cout) gives the bits of the same residual passed dense."""
    K, x, w = _conv_operands(cuda)
    B, H, W, Cout = 2, 9, 7, 64
    g = torch.Generator().manual_seed(6)
    wide = torch.randn(B * H * W, Cout + 24, generator=g).to(K.ELEM).to(cuda)
    res = wide[:, 8:8 + Cout].view(B, H, W, Cout)
    assert not res.is_contiguous()
    got = K.conv2d(x, w, resid=res)
    want = K.conv2d(x, w, resid=res.contiguous())
    assert torch.equal(got, want)
    plain = K.conv2d(x, w)
    assert not torch.equal(got, plain)
