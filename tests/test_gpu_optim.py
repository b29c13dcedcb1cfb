"""Direct tests of the optimizer tail (csrc/optim.hip): the gradient norm / clip coefficient, the fused AdamW step
and the fp32 zero fill, against float64 restatements on the CPU.

The sizes are the ones at which sqnorm_partial_kernel / adamw_kernel / zero_kernel change path: below one float4, a
ragged n % 4 tail, more than one block, more elements than the 2048 x 256 threads of the capped grid (a second
grid-stride trip; the 16-byte-aligned float4 path of the norm needs 4 x as many for it), and a 4-byte-misaligned
buffer (`buf[1:]`), which takes the norm's scalar path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = 2048 * 256  # threads of the capped grid (nblocks() in csrc/optim.hip)
SIZES = [1, 3, 4, 1027,
         GRID * 2 + 5,        # scalar path: second and third grid-stride trip
         4 * (GRID + 3) + 3]  # float4 path: second trip of three vectors, then a 3-element tail
F32 = np.float32


def _grad(n, misaligned, seed, scale, dev):
    """Seeded standard normal * scale as a length-n device view: 256-byte aligned, or 4 bytes past it."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale
    buf = torch.empty(n + 1, device=dev)
    view = buf[1:] if misaligned else buf[:n]
    view.copy_(g)
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return g, view


def _want_coef(norm, max_norm):
    """torch's clip_grad_norm_ coefficient in float32 from the kernel's own norm."""
    if max_norm <= 0:
        return F32(1)
    return min(F32(1), F32(max_norm) / (F32(norm) + F32(1e-6)))


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_clip_coef_vs_float64_norm(cuda, n, misaligned):
    """out[0] = ||g|| grad_scale within rtol 2e-7 of torch.linalg.vector_norm(g.double()) (the sum is fp64; one fp32
    rounding of the sqrt and one of the product, 2 x 2^-24 = 1.2e-7); out[1] = min(1, max_norm / (out[0] + 1e-6))
    in fp32 from the kernel's own out[0], bit for bit; max_norm <= 0 gives exactly 1; `out=` is honoured."""
    from pairwise_sample_optimization_amd import kernels as K
    for gs in (1.0 / 65536, 0.25):
        g, view = _grad(n, misaligned, n, 3.0 / gs, cuda)  # scaled norm about 3 sqrt(n): clips at max_norm 1
        want = float(torch.linalg.vector_norm(g.double())) * gs
        for max_norm in (1.0, 100.0 * want, 0.0, -1.0):
            out = torch.full((2,), -7.0, device=cuda)
            ret = K.grad_clip_coef(view, max_norm, grad_scale=gs, out=out)
            assert ret is out
            norm, coef = out.cpu().numpy()
            assert abs(float(norm) - want) <= 2e-7 * want, (norm, want)
            assert coef.tobytes() == _want_coef(norm, max_norm).tobytes(), (coef, _want_coef(norm, max_norm))
            if max_norm <= 0 or max_norm > want:
                assert coef == 1.0
        fresh = K.grad_clip_coef(view, 1.0, grad_scale=gs).cpu().numpy()
        assert fresh.shape == (2,) and fresh[0] == F32(norm)
        if n >= 4:
            assert fresh[1] < 1.0  # 3 sqrt(n) is far above max_norm 1: the clipping branch ran


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", [1027, GRID * 2 + 5])
def test_grad_clip_norm_reports_a_non_finite_gradient(cuda, n, misaligned):
    """One inf, and separately one nan, at element 0, at the last element of the float4 body, in the ragged tail, and
    at elements that the last block / the later grid-stride trips read: the returned norm is non-finite every time.
    The fp16 loss-scaling skip reads exactly this value."""
    from pairwise_sample_optimization_amd import kernels as K
    _, view = _grad(n, misaligned, 7, 1.0, cuda)
    spots = {0, (n // 4) * 4 - 1, n - 1, n // 2}
    if n > GRID:
        spots |= {GRID - 1, GRID, 2 * GRID - 1, 2 * GRID, 4 * ((n // 4) - 1)}
    assert np.isfinite(K.grad_clip_coef(view, 1.0, grad_scale=0.25).cpu().numpy()).all()
    for pos in sorted(spots):
        keep = view[pos].clone()
        for bad in (float("inf"), float("-inf"), float("nan")):
            view[pos] = bad
            for gs in (0.25, 1.0 / 65536):
                norm = K.grad_clip_coef(view, 1.0, grad_scale=gs)[0].item()
                assert not np.isfinite(norm), (pos, bad, gs, norm)
        view[pos] = keep
    assert np.isfinite(K.grad_clip_coef(view, 1.0, grad_scale=0.25).cpu().numpy()).all()


# hyper-parameters as the C ABI receives them (float): the float64 restatement uses the same values
LR, B1, B2, EPS = (float(F32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))


def _adamw_ref(p, g, m, v, step, wd, s):
    """Decoupled AdamW (torch.optim.AdamW's update) in float64 on gradient g * s."""
    gi = g * s
    p = p * (1.0 - LR * wd)
    m = B1 * m + (1.0 - B1) * gi
    v = B2 * v + (1.0 - B2) * gi * gi
    denom = np.sqrt(v) / np.sqrt(1.0 - B2 ** step) + EPS
    return p - LR / (1.0 - B1 ** step) * (m / denom), m, v


@pytest.mark.parametrize("clipped", [True, False], ids=["scale0.25-clip", "scale1-noclip"])
@pytest.mark.parametrize("wd", [0.0, float(F32(1e-2))], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("n", [10_007, GRID + 3])
def test_adamw_step_vs_float64(cuda, n, wd, clipped, capsys):
    """Five steps of pso_adamw_step against the float64 restatement, fresh gradients every step, either with
    grad_scale = 0.25 and the clip tensor of pso_grad_clip_coef (its coefficient is checked above; the restatement
    takes the kernel's value) or with clip=None and grad_scale = 1.  p, m and v within 1e-6 max|ref|, the scale of the
    trainer test's 1e-5 absolute bound on unit-scale parameters: five steps of two float32 roundings each on p
    (the decay product and the update) are 10 x 2^-24 = 6e-7 at worst.  Observed on an MI355X, largest over the
    cases: p 3.3e-7 (wd = 1e-2; 1.4e-7 without decay), m 1.4e-7, v 1.2e-7."""
    from pairwise_sample_optimization_amd import kernels as K
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    p, m, v = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    rp, rm, rv = p0.double().numpy(), np.zeros(n), np.zeros(n)
    gs = 0.25 if clipped else 1.0
    for step in range(1, 6):
        g = torch.randn(n, generator=gen) * 3
        gd = g.to(cuda)
        clip = K.grad_clip_coef(gd, 1.0, grad_scale=gs) if clipped else None
        K.adamw_step(p, gd, m, v, LR, (B1, B2), EPS, wd, step, grad_scale=gs, clip=clip)
        s = gs * (float(clip[1].item()) if clipped else 1.0)
        if clipped:
            assert clip[1].item() < 1.0
        rp, rm, rv = _adamw_ref(rp, g.double().numpy(), rm, rv, step, wd, s)
    rel = {}
    for name, got, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
        rel[name] = np.abs(got.cpu().double().numpy() - ref).max() / np.abs(ref).max()
    with capsys.disabled():
        print(f"\n  [adamw n={n} wd={wd:g} clipped={clipped}] max|diff| / max|ref|: " +
              "  ".join(f"{k} {e:.2e}" for k, e in rel.items()))
    assert np.abs(rp - p0.double().numpy()).max() > 1e-3  # the parameters moved
    for name, e in rel.items():
        assert e <= 1e-6, (name, e)


def test_adamw_step_rejects_step_zero(cuda):
    from pairwise_sample_optimization_amd import kernels as K, _lib
    t = torch.zeros(8, device=cuda)
    with pytest.raises(_lib.PsoLibError):
        K.adamw_step(t, t.clone(), t.clone(), t.clone(), LR, (B1, B2), EPS, 0.0, 0)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", [1, SIZES[-1]])
def test_zero_fills_the_view_and_nothing_else(cuda, n, misaligned):
    """Every element of the view is +0.0 by bits; the guard elements around it keep theirs."""
    from pairwise_sample_optimization_amd import kernels as K
    off = 1 if misaligned else 0
    buf = torch.randn(n + 2, generator=torch.Generator().manual_seed(n)).abs().neg().sub(1.0).to(cuda)  # all < -1
    before = buf.clone()
    view = buf[off: off + n]
    assert K.zero_(view) is view
    assert (view.view(torch.int32) == 0).all()
    assert torch.equal(buf[:off], before[:off]) and torch.equal(buf[off + n:], before[off + n:])
