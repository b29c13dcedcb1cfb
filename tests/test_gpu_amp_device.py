"""Kernel-level GPU cases of the device-resident loss scaler (include/pso_amd.h PSO_AMP_*, csrc/optim.hip): the scale
state machine against the numbers tests/test_f16_build.py pins for amp.LossScaler, the unscale / norm / clip finalize
against K.grad_clip_coef, found_inf on every load path of the norm kernel, the skipped step and the applied step of the
`_amp` optimizer entries against the host-argument entries.  fp32 / integer arithmetic only: these run on the default
(bf16) library; the trainers' cases run under PSO_LIB=f16 (tests/test_gpu_f16_amp.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.999)
LR, EPS, WD = 1e-3, 1e-8, 1e-2


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _scaler(cuda, **kw):
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    return DeviceLossScaler(device=cuda, **kw)


def _words(sc):
    """The state block on the host: (int32 words, the same bytes as float32)."""
    h = sc.state.cpu()
    return h, h.view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_state_machine_matches_the_host_scaler(cuda):
    """unscale/clip + update over the overflow pattern of tests/test_f16_build.py (growth interval 3), an inf planted
    in a 1003-element gradient on the overflow steps.  Scales are powers of two: the comparison is exact."""
    from pairwise_sample_optimization_amd import _lib, kernels as K
    from pairwise_sample_optimization_amd.amp import LossScaler
    pattern = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    want = [65536, 65536, 32768, 32768, 32768, 65536, 32768, 16384, 16384, 16384, 32768, 32768]
    sc = _scaler(cuda, growth_interval=3)
    host = LossScaler(growth_interval=3)
    clean = torch.randn(1003, device=cuda, generator=_gen(0))
    scales, skipped_at, applied = [], [], 0
    for i, inf in enumerate(pattern, 1):
        g = clean.clone()
        if inf:
            g[500] = float("inf")
        K.amp_unscale_clip(g, 1.0, sc.state, BETAS)
        found = int(_words(sc)[0][_lib.AMP_FOUND_INF])
        K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)
        host.update(bool(inf))
        assert found == inf, i
        applied += 1 - inf
        if inf:
            skipped_at.append(i)
        scales.append(sc.scale)
        wi, wf = _words(sc)
        assert sc.scale == host.scale and sc.growth_tracker == host.growth_tracker and sc.skipped == host.skipped
        assert sc.step == applied and wf[_lib.AMP_INV_SCALE].item() == 1.0 / host.scale
    assert scales == [float(s) for s in want]
    assert skipped_at == [3, 7, 8] and sc.skipped == 3 and sc.step == 9
    sd = sc.state_dict()
    assert sd["scale"] == 32768.0 and sd["growth_tracker"] == host.growth_tracker and sd["step"] == 9
    other = _scaler(cuda)
    other.load_state_dict(sd)
    assert torch.equal(other.state[:_lib.AMP_NORM], sc.state[:_lib.AMP_NORM]) and other.growth_interval == 3


@pytest.mark.parametrize("S", [2.0 ** 16, 2.0 ** 3])
@pytest.mark.parametrize("gs", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("shape", ["n1003", "n11243", "unaligned"])
def test_norm_and_coefficient_are_the_host_divided_bits(cuda, S, gs, shape):
    """norm and clip coefficient == K.grad_clip_coef(grad, max_norm, grad_scale=gs / S) bit for bit: S is a power of
    two, so fp32(gs) * fp32(1 / S) is fp32(gs / S) exactly and the two kernels evaluate the same expression.  n = 1003
    (one ragged block), 2048 * 5 + 1003 (more than one block per thread stride), and grad[1:] (4-B aligned only: the
    scalar path)."""
    from pairwise_sample_optimization_amd import _lib, kernels as K
    n = {"n1003": 1003, "n11243": 2048 * 5 + 1003, "unaligned": 1004}[shape]
    grad = torch.randn(n, device=cuda, generator=_gen(n)) * S * 3.0  # a scaled gradient whose true norm clips
    if shape == "unaligned":
        grad = grad[1:]
        assert grad.data_ptr() % 16 == 4
    for max_norm in (1.0, 1e6, 0.0):  # clipping, not clipping, clipping off
        ref = K.grad_clip_coef(grad, max_norm, grad_scale=gs / S)
        sc = _scaler(cuda, init_scale=S)
        K.amp_unscale_clip(grad, max_norm, sc.state, BETAS, grad_scale=gs)
        wi, wf = _words(sc)
        got = torch.stack([wf[_lib.AMP_NORM], wf[_lib.AMP_CLIP_COEF]])
        assert torch.equal(_bits(got), _bits(ref.cpu())), (max_norm, got, ref)
        assert wi[_lib.AMP_FOUND_INF] == 0 and wi[_lib.AMP_STEP] == 1
        assert _bits(wf[_lib.AMP_GRAD_MUL:_lib.AMP_GRAD_MUL + 1]).item() == \
            _bits(torch.tensor([gs / S], dtype=torch.float32)).item()
    assert 0.0 < ref[0].item() < float("inf")


@pytest.mark.parametrize("case", ["inf_last_of_ragged_tail", "nan_first_vector", "finite_overflowing_norm",
                                  "inf_unaligned_scalar_path"])
def test_found_inf_reaches_every_load_path(cuda, case):
    from pairwise_sample_optimization_amd import _lib, kernels as K
    n = 2048 * 5 + 1003  # 16-B vectors, then a 3-element scalar tail
    grad = torch.randn(n, device=cuda, generator=_gen(1))
    if case == "inf_last_of_ragged_tail":
        grad[n - 1] = float("inf")
    elif case == "nan_first_vector":
        grad[1] = float("nan")
    elif case == "finite_overflowing_norm":
        grad.fill_(3e38)  # every element finite; the fp64 sum's root is beyond fp32
        assert torch.isfinite(grad).all()
    else:
        grad = grad[1:]
        grad[7] = float("-inf")
    sc = _scaler(cuda, init_scale=1.0)
    K.amp_unscale_clip(grad, 1.0, sc.state, BETAS)
    wi, wf = _words(sc)
    assert wi[_lib.AMP_FOUND_INF] == 1 and wi[_lib.AMP_STEP] == 0 and not torch.isfinite(wf[_lib.AMP_NORM])
    # and a clean gradient clears it again
    K.amp_unscale_clip(torch.ones(n, device=cuda), 1.0, sc.state, BETAS)
    wi, _ = _words(sc)
    assert wi[_lib.AMP_FOUND_INF] == 0 and wi[_lib.AMP_STEP] == 1


def _adam8(cuda):
    """Two tensors in one flat buffer: 2048 * 5 + 1003 elements (8-bit state, ragged last block) and 1000 elements
    (under min_8bit_size: 32-bit state), the second at a 16-B aligned offset behind a pad."""
    from pairwise_sample_optimization_amd import kernels as K
    n1, n2 = 2048 * 5 + 1003, 1000
    off2 = -(-n1 // 8) * 8
    n = off2 + n2
    return n, [(0, n1), (off2, n2)], K.Adam8State(n, cuda, segments=[(0, n1), (off2, n2)])


def _covered(n, segs, device):
    m = torch.zeros(n, dtype=torch.bool, device=device)
    for o, k in segs:
        m[o:o + k] = True
    return m


def test_skipped_step_leaves_everything_unchanged(cuda):
    """After a found_inf step parameters, m / v, codes, absmax, 32-bit state and the 16-bit working copy are bitwise
    unchanged, the zero_grad form has zeroed the gradient it covers, and the step count did not advance."""
    from pairwise_sample_optimization_amd import _lib, kernels as K
    g = _gen(2)
    # ---- fp32 AdamW, n = 1003
    n = 1003
    p, m, v = (torch.randn(n, device=cuda, generator=g) for _ in range(3))
    v = v.abs()
    grad = torch.randn(n, device=cuda, generator=g)
    grad[n - 1] = float("inf")
    sc = _scaler(cuda, init_scale=1024.0)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    K.amp_unscale_clip(grad, 1.0, sc.state, BETAS)
    K.adamw_step(p, grad, m, v, LR, BETAS, EPS, WD, amp_state=sc.state)
    K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(_bits(a), _bits(b))
    assert sc.step == 0 and sc.skipped == 1 and sc.scale == 512.0
    # ---- 8-bit per-tensor AdamW, with and without the folded zero_grad
    for zero_grad in (False, True):
        n, segs, st = _adam8(cuda)
        sc = _scaler(cuda, init_scale=1024.0)
        p = torch.randn(n, device=cuda, generator=g) * 0.02
        work = K.cast_f32_bf16(p)
        warm = torch.randn(n, device=cuda, generator=g) * 1e-2
        K.amp_unscale_clip(warm, 1.0, sc.state, BETAS)  # one applied step first: non-trivial codes / absmax / m32
        K.adamw8bit_step(p, warm, st, LR, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work)
        assert sc.step == 1 and st.am.abs().max().item() > 0 and st.m32.abs().max().item() > 0
        before = {k: t.clone() for k, t in st.tensors().items()}
        p0, w0 = p.clone(), work.clone()
        grad = torch.randn(n, device=cuda, generator=g)
        grad[2048 * 5 + 1002] = float("inf")
        g0 = grad.clone()
        K.amp_unscale_clip(grad, 1.0, sc.state, BETAS)
        zeroed = K.adamw8bit_step(p, grad, st, LR, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work,
                                  zero_grad=zero_grad)
        K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)
        assert zeroed == zero_grad
        assert torch.equal(_bits(p), _bits(p0)) and torch.equal(work.view(torch.int16), w0.view(torch.int16))
        for k, t in st.tensors().items():
            assert torch.equal(t, before[k]), k
        cov = _covered(n, segs, cuda)
        if zero_grad:
            assert grad[cov].abs().max().item() == 0.0
            assert torch.equal(_bits(grad[~cov]), _bits(g0[~cov]))  # the pad between the tensors is not touched
        else:
            assert torch.equal(_bits(grad), _bits(g0))
        assert sc.step == 1 and sc.skipped == 1 and sc.scale == 512.0


def test_applied_steps_match_the_host_argument_entries(cuda):
    """Steps 1..3 on the same inputs through the `_amp` entries (S = 1024, 1/world = 1/3, clipping on) and through
    pso_adamw_step / pso_adamw8bit_step (zero_grad) with host arguments.  m / v, codes, absmax and the 32-bit
    state do not depend on the bias correction: bit-identical.  Parameters: the device evaluates the bias-correction
    formulas with its own powf / pow, so they are held to 1e-6 * max|p| (the bar of the 8-bit restatement test,
    DESIGN.md section 7 #4); the number of differing elements is printed."""
    from pairwise_sample_optimization_amd import kernels as K
    S, gs, max_norm = 1024.0, 1.0 / 3.0, 1.0
    g = _gen(3)
    # ---- fp32 AdamW
    n = 1003
    p_a = torch.randn(n, device=cuda, generator=g)
    m_a, v_a = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    p_h, m_h, v_h = p_a.clone(), m_a.clone(), v_a.clone()
    sc = _scaler(cuda, init_scale=S)
    for step in (1, 2, 3):
        grad = torch.randn(n, device=cuda, generator=g) * S
        K.amp_unscale_clip(grad, max_norm, sc.state, BETAS, grad_scale=gs)
        K.adamw_step(p_a, grad, m_a, v_a, LR, BETAS, EPS, WD, amp_state=sc.state)
        K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)
        clip = K.grad_clip_coef(grad, max_norm, grad_scale=gs / S)
        K.adamw_step(p_h, grad, m_h, v_h, LR, BETAS, EPS, WD, step, grad_scale=gs / S, clip=clip)
        assert torch.equal(_bits(m_a), _bits(m_h)) and torch.equal(_bits(v_a), _bits(v_h)), step
        d = (p_a - p_h).abs().max().item() / p_h.abs().max().item()
        print(f"  fp32 AdamW step {step}: {(p_a != p_h).sum().item()} of {n} parameters differ, max {d:.2e} of max|p|")
        assert d <= 1e-6
    assert sc.step == 3
    # ---- 8-bit per-tensor AdamW (zero_grad folded), with the 16-bit working copy
    n, segs, st_a = _adam8(cuda)
    _, _, st_h = _adam8(cuda)
    p_a = torch.randn(n, device=cuda, generator=g) * 0.02
    p_h = p_a.clone()
    w_a, w_h = K.cast_f32_bf16(p_a), K.cast_f32_bf16(p_h)
    sc = _scaler(cuda, init_scale=S)
    for step in (1, 2, 3):
        grad = torch.randn(n, device=cuda, generator=g) * S * 1e-2
        g_h = grad.clone()
        K.amp_unscale_clip(grad, max_norm, sc.state, BETAS, grad_scale=gs)
        K.adamw8bit_step(p_a, grad, st_a, LR, BETAS, EPS, WD, amp_state=sc.state, out_bf16=w_a, zero_grad=True)
        K.amp_update(sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval)
        clip = K.grad_clip_coef(g_h, max_norm, grad_scale=gs / S)
        K.adamw8bit_step(p_h, g_h, st_h, LR, BETAS, EPS, WD, step, grad_scale=gs / S, clip=clip, out_bf16=w_h,
                         zero_grad=True)
        for (k, a), b in zip(st_a.tensors().items(), st_h.tensors().values()):
            assert torch.equal(a, b), (step, k)
        assert torch.equal(_bits(grad), _bits(g_h))  # both zeroed what they cover
        d = (p_a - p_h).abs().max().item() / p_h.abs().max().item()
        print(f"  8-bit AdamW step {step}: {(p_a != p_h).sum().item()} of {n} parameters differ, max {d:.2e} of max|p|")
        assert d <= 1e-6
        assert torch.equal(w_a.view(torch.int16), K.cast_f32_bf16(p_a).view(torch.int16))
    assert sc.step == 3 and sc.skipped == 0
