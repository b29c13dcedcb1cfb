"""GPU cases of the learning-rate schedule on the default (bf16) library: pso_lr_schedule against the host LrSchedule,
the optimizer steps with the lr in a device word against the same steps with the float, and the trainers' optimizer
step with a schedule.  fp32 / fp64 / integer arithmetic only; the device-scaler trainer cases run under PSO_LIB=f16
(tests/test_gpu_lr_schedule_f16.py).

Bounds.  pso_lr_schedule evaluates the host's double expressions on the device and rounds to fp32 once, as the host
does.  Where the expression is integer conversions, IEEE divisions and one multiplication (constant, the warm-up ramp,
the linear decay) both sides form the same double: bit-equal.  Where it calls cos or pow, the device's double result may
differ from libm's in its last bits, which moves the fp32 rounding by at most one step: 1 fp32 ulp.
The steps with a device lr word run the host-argument kernels with the lr loaded instead of passed: bit-identical.
The trainer against its K.adamw_step mirror: the same entry with the same arguments, bit-identical; against CPU
torch.optim.AdamW with the transformers scheduler: the 1e-5 absolute bound of
tests/test_gpu_trainer.py::test_optimizer_step_matches_torch_adamw."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from prodigy_ref import ProdigyRef

pytestmark = pytest.mark.gpu

KINDS = ["constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial"]
EXACT = ("constant", "constant_with_warmup", "linear")
W, T = 3, 12
BETAS = (0.9, 0.999)
LR, EPS, WD = 1e-3, 1e-8, 1e-2
N = 2048 * 5 + 1003  # a 16-byte body and a 3-element tail


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scaler(cuda, **kw):
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    return DeviceLossScaler(device=cuda, **kw)


def _set_words(sc, **words):
    """Host-side fill of integer / float words of the scaler's block (no non-finite arithmetic on the device)."""
    from pairwise_sample_optimization_amd import _lib
    host = sc.state.cpu()
    for name, val in words.items():
        w = getattr(_lib, "AMP_" + name)
        if w in _lib.AMP_INT_WORDS:
            host[w] = int(val)
        else:
            host.view(torch.float32)[w] = float(val)
    sc.state.copy_(host)


def _f32_bits(x):
    return int(np.array([x], dtype=np.float64).astype(np.float32).view(np.int32)[0])


# ----------------------------------------------------------------------------------------------------------------------
# 1. pso_lr_schedule
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_device_schedule_matches_the_host(cuda, kind):
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    sched = LrSchedule(kind, 2e-4, W, T, num_cycles=2, power=2.0)
    ks = list(range(16))
    out = torch.zeros(len(ks), device=cuda)
    out_st = torch.zeros(len(ks), device=cuda)
    sc = _scaler(cuda)
    for k in ks:
        K.lr_schedule(sched, out[k:k + 1], step=k + 1)
        _set_words(sc, STEP=k + 1, FOUND_INF=0)  # what pso_amp_unscale_clip leaves for the (k + 1)-th applied step
        K.lr_schedule(sched, out_st[k:k + 1], step=12345, amp_state=sc.state)  # `step` is not read with a state
    got = _bits(out).cpu().tolist()
    want = [_f32_bits(sched.lr(k)) for k in ks]
    ulps = [abs(a - b) for a, b in zip(got, want)]
    print(f"  {kind}: max fp32 ulp distance {max(ulps)} over k = 0..15; lr {out.cpu().tolist()}")
    assert all(np.isfinite(out.cpu().numpy())) and out.min().item() >= 0.0
    if kind in EXACT:
        assert got == want
    else:
        for k in ks:
            if k < W:
                assert got[k] == want[k], k  # the warm-up ramp
        assert max(ulps) <= 1, list(zip(ks, got, want))
    assert _bits(out_st).cpu().tolist() == got  # the state's step count gives the bits of the explicit-step call
    if kind != "constant":
        assert got[0] == 0  # every warm-up starts at lr = +0.0
    # FOUND_INF: the word is left as it was
    sentinel = torch.full((1,), 123.25, device=cuda)
    _set_words(sc, STEP=5, FOUND_INF=1)
    K.lr_schedule(sched, sentinel, amp_state=sc.state)
    assert sentinel.item() == 123.25
    _set_words(sc, FOUND_INF=0)
    K.lr_schedule(sched, sentinel, amp_state=sc.state)
    assert _bits(sentinel).item() == got[4]


def test_schedule_argument_errors(cuda):
    from pairwise_sample_optimization_amd import _lib, kernels as K
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    sched = LrSchedule("linear", 1e-3, 2, 6)
    out = torch.full((1,), 7.0, device=cuda)
    with pytest.raises(_lib.PsoLibError, match="step"):
        K.lr_schedule(sched, out, step=0)
    with pytest.raises(_lib.PsoLibError):
        K.lr_schedule(sched, out)
    with pytest.raises(_lib.PsoLibError, match="float32"):
        K.lr_schedule(sched, torch.zeros(2, device=cuda), step=1)
    with pytest.raises(_lib.PsoLibError, match="kind"):
        _lib.check(_lib.lib().pso_lr_schedule(9, 1e-3, 2, 6, 1, 1.0, None, 1, out.data_ptr(), _lib.stream_ptr()))
    assert out.item() == 7.0


# ----------------------------------------------------------------------------------------------------------------------
# 2. the lr in a device word against the float argument
# ----------------------------------------------------------------------------------------------------------------------
def _word(cuda, lr):
    return torch.tensor([lr], dtype=torch.float32, device=cuda)


def _amp_state(cuda, grad, S=1024.0, gs=1.0 / 3.0, steps_before=2):
    """A scaler block after pso_amp_unscale_clip on `grad` (clipping on): GRAD_MUL, CLIP_COEF and the bias corrections
    of step steps_before + 1."""
    from pairwise_sample_optimization_amd import kernels as K
    sc = _scaler(cuda, init_scale=S)
    _set_words(sc, STEP=steps_before)
    K.amp_unscale_clip(grad, 1.0, sc.state, BETAS, grad_scale=gs)
    return sc


@pytest.mark.parametrize("lr", [LR, 0.0])
@pytest.mark.parametrize("misaligned", [False, True])
def test_adamw_lr_entry_is_the_host_argument_entry(cuda, lr, misaligned):
    """lr = 0 (legal at run time only through the word): parameters bit-unchanged, moments moved."""
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(5)
    n = N + (1 if misaligned else 0)
    mk = lambda: torch.randn(n, device=cuda, generator=g)
    p, m, v, grad = mk(), mk() * 1e-2, mk().abs() * 1e-4, mk() * 1024.0
    if misaligned:  # [1:] views: 4-byte aligned only, the scalar path
        p, m, v, grad = (t[1:] for t in (p, m, v, grad))
        assert all(t.data_ptr() % 16 == 4 for t in (p, m, v, grad))
    sc = _amp_state(cuda, grad)
    a = [t.clone() for t in (p, m, v)]
    b = [t.clone() for t in (p, m, v)]
    if misaligned:
        a = [torch.empty(N + 1, device=cuda)[1:].copy_(t) for t in a]
        b = [torch.empty(N + 1, device=cuda)[1:].copy_(t) for t in b]
        assert all(t.data_ptr() % 16 == 4 for t in a + b)
    K.adamw_step(a[0], grad, a[1], a[2], _word(cuda, lr), BETAS, EPS, WD, amp_state=sc.state)
    K.adamw_step(b[0], grad, b[1], b[2], lr, BETAS, EPS, WD, amp_state=sc.state)
    for x, y, name in zip(a, b, "pmv"):
        assert torch.equal(_bits(x), _bits(y)), name
    assert not torch.equal(a[1], m) and not torch.equal(a[2], v)  # the moments moved
    if lr == 0.0:
        assert torch.equal(_bits(a[0]), _bits(p))
    else:
        assert not torch.equal(a[0], p)


def _adam8(cuda):
    """tests/test_gpu_amp_device.py::_adam8: one tensor of 2048 * 5 + 1003 elements (8-bit state, ragged last block)
    and one of 1000 (under min_8bit_size: 32-bit state) behind a pad."""
    from pairwise_sample_optimization_amd import kernels as K
    n1, n2 = N, 1000
    off2 = -(-n1 // 8) * 8
    n = off2 + n2
    segs = [(0, n1), (off2, n2)]
    return n, segs, K.Adam8State(n, cuda, segments=segs)


def _covered(n, segs, device):
    m = torch.zeros(n, dtype=torch.bool, device=device)
    for o, k in segs:
        m[o:o + k] = True
    return m


@pytest.mark.parametrize("lr", [LR, 0.0])
@pytest.mark.parametrize("zero_grad", [False, True])
def test_adamw8bit_lr_entries_are_the_host_argument_entries(cuda, lr, zero_grad):
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(6)
    n, segs, st_a = _adam8(cuda)
    _, _, st_b = _adam8(cuda)
    p0 = torch.randn(n, device=cuda, generator=g) * 0.02
    warm = torch.randn(n, device=cuda, generator=g) * 1e-2
    grad = torch.randn(n, device=cuda, generator=g) * 1024.0 * 1e-2
    sc = _scaler(cuda, init_scale=1.0)
    runs = []
    for st, lr_arg in ((st_a, _word(cuda, lr)), (st_b, lr)):
        p = p0.clone()
        work = K.cast_f32_bf16(p)
        _set_words(sc, STEP=0, SCALE=1.0, INV_SCALE=1.0)
        K.amp_unscale_clip(warm, 1.0, sc.state, BETAS)  # one applied step first: non-trivial codes / absmax / m32
        K.adamw8bit_step(p, warm.clone(), st, LR, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work)
        before = {k: t.clone() for k, t in st.tensors().items()}
        p1 = p.clone()
        _set_words(sc, SCALE=1024.0, INV_SCALE=1.0 / 1024.0)
        gr = grad.clone()
        K.amp_unscale_clip(gr, 1.0, sc.state, BETAS, grad_scale=1.0 / 3.0)
        zeroed = K.adamw8bit_step(p, gr, st, lr_arg, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work,
                                  zero_grad=zero_grad)
        assert zeroed == zero_grad
        runs.append((p, work, gr, {k: t.clone() for k, t in st.tensors().items()}, before, p1))
    (pa, wa, ga, sa, before, p1), (pb, wb, gb, sb, _, _) = runs
    assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(wa.view(torch.int16), wb.view(torch.int16))
    assert torch.equal(_bits(ga), _bits(gb))
    for k in sa:  # codes, absmax, 32-bit state, block table
        assert torch.equal(sa[k], sb[k]), k
    cov = _covered(n, segs, cuda)
    if zero_grad:
        assert ga[cov].abs().max().item() == 0.0 and torch.equal(_bits(ga[~cov]), _bits(grad[~cov]))
    else:
        assert torch.equal(_bits(ga), _bits(grad))
    assert not torch.equal(sa["exp_avg_q"], before["exp_avg_q"]) and not torch.equal(sa["exp_avg_32"],
                                                                                     before["exp_avg_32"])
    if lr == 0.0:
        assert torch.equal(_bits(pa), _bits(p1))
    else:
        assert not torch.equal(pa[cov], p1[cov])


def test_lr_entries_skip_on_found_inf(cuda):
    """FOUND_INF set by a host-side fill: nothing is written except the zeroed gradient of the zero_grad form."""
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(7)
    word = _word(cuda, LR)
    # fp32 AdamW
    p, m, v, grad = (torch.randn(N, device=cuda, generator=g) for _ in range(4))
    v = v.abs()
    sc = _amp_state(cuda, grad)
    _set_words(sc, FOUND_INF=1)
    keep = [t.clone() for t in (p, m, v, grad)]
    K.adamw_step(p, grad, m, v, word, BETAS, EPS, WD, amp_state=sc.state)
    for x, y in zip((p, m, v, grad), keep):
        assert torch.equal(_bits(x), _bits(y))
    # 8-bit, both forms
    for zero_grad in (False, True):
        n, segs, st = _adam8(cuda)
        p = torch.randn(n, device=cuda, generator=g) * 0.02
        work = K.cast_f32_bf16(p)
        warm = torch.randn(n, device=cuda, generator=g) * 1e-2
        sc = _scaler(cuda, init_scale=1.0)
        K.amp_unscale_clip(warm, 1.0, sc.state, BETAS)
        K.adamw8bit_step(p, warm, st, word, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work)
        assert st.am.abs().max().item() > 0 and st.m32.abs().max().item() > 0
        before = {k: t.clone() for k, t in st.tensors().items()}
        p1, w1 = p.clone(), work.clone()
        grad = torch.randn(n, device=cuda, generator=g)
        g0 = grad.clone()
        _set_words(sc, FOUND_INF=1)
        K.adamw8bit_step(p, grad, st, word, BETAS, EPS, WD, amp_state=sc.state, out_bf16=work, zero_grad=zero_grad)
        assert torch.equal(_bits(p), _bits(p1)) and torch.equal(work.view(torch.int16), w1.view(torch.int16))
        for k, t in st.tensors().items():
            assert torch.equal(t, before[k]), k
        cov = _covered(n, segs, cuda)
        if zero_grad:
            assert grad[cov].abs().max().item() == 0.0 and torch.equal(_bits(grad[~cov]), _bits(g0[~cov]))
        else:
            assert torch.equal(_bits(grad), _bits(g0))
    assert word.item() == np.float32(LR)


@pytest.mark.parametrize("opt", ["adamw", "adamw8bit"])
def test_device_lr_word_without_amp_state_is_the_host_float(cuda, opt):
    """lr from the device word with the step count, grad_scale and clip from the host (no amp_state): three steps at
    lr 0, 1e-3 and float32(2e-4 / 3), each bit-identical to the same call with the float -- parameters, moments or
    codes, absmax, 32-bit state and the bf16 copy.  At lr 0 the parameters keep their bits while the moments move.
    fp32 AdamW over 4101 elements; the 8-bit step over a block table of 3000 (32-bit state) + 4101 (8-bit, a
    5-element last block) elements."""
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(11)
    lrs = [0.0, 1e-3, float(np.float32(2e-4 * (1 / 3)))]
    segs = [(0, 3000), (3000, 4101)]
    n = 4101 if opt == "adamw" else 3000 + 4101
    p0 = torch.randn(n, device=cuda, generator=g) * 0.02
    grads = [torch.randn(n, device=cuda, generator=g) * 1e-2 for _ in lrs]
    clips = [K.grad_clip_coef(gr, 0.5, grad_scale=1.0 / 3.0) for gr in grads]

    def run(as_word):
        p, out = p0.clone(), []
        if opt == "adamw":
            state = {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        else:
            st = K.Adam8State(n, cuda, segments=segs)
            work = K.cast_f32_bf16(p)
            state = dict(st.tensors(), work=work)
        for step, (lr, gr, clip) in enumerate(zip(lrs, grads, clips), 1):
            lr_arg = _word(cuda, lr) if as_word else lr
            gr = gr.clone()
            if opt == "adamw":
                K.adamw_step(p, gr, state["exp_avg"], state["exp_avg_sq"], lr_arg, BETAS, EPS, WD, step,
                             grad_scale=1.0 / 3.0, clip=clip)
            else:
                K.adamw8bit_step(p, gr, st, lr_arg, BETAS, EPS, WD, step, grad_scale=1.0 / 3.0, clip=clip,
                                 out_bf16=work, zero_grad=step == 2)
            out.append(dict({k: t.clone() for k, t in state.items()}, param=p.clone(), grad=gr))
        return out

    word, host = run(True), run(False)
    for step, (a, b) in enumerate(zip(word, host), 1):
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (step, k)
    assert torch.equal(_bits(word[0]["param"]), _bits(p0))  # lr 0: the parameters keep their bits ...
    moved = ("exp_avg_q", "exp_avg_sq_q", "exp_avg_32", "exp_avg_sq_32")
    for k in ("exp_avg", "exp_avg_sq") if opt == "adamw" else moved:  # ... while the moments move
        assert word[0][k].any(), k
    assert not torch.equal(word[1]["param"], p0) and not torch.equal(word[2]["param"], word[1]["param"])
    if opt == "adamw8bit":
        assert word[1]["grad"].abs().max().item() == 0.0 and torch.equal(word[0]["grad"], grads[0])


@pytest.mark.parametrize("misaligned", [False, True])
def test_prodigy_lr_entry_is_the_host_argument_entry(cuda, misaligned):
    """Three steps, with and without the scaler's block (amp_state may be NULL), p, m, v, s and the state block
    compared as bytes."""
    from pairwise_sample_optimization_amd import kernels as K
    n = N

    def view(x):
        buf = torch.empty(n + 1, device=cuda)
        out = buf[1:] if misaligned else buf[:n]
        out.copy_(x)
        assert out.data_ptr() % 16 == (4 if misaligned else 0)
        return out

    gen = torch.Generator().manual_seed(9)
    p0 = 1e-2 * torch.randn(n, generator=gen)
    c = torch.randn(n, generator=gen)
    grads = [view(c + 0.3 * torch.randn(n, generator=gen)) for _ in range(3)]
    hyp = dict(use_bias_correction=True, safeguard_warmup=True, d_coef=4.0)
    for amp in (False, True):
        sc = _amp_state(cuda, grads[0], S=8.0) if amp else None
        runs = []
        for form in ("word", "float"):
            p = view(p0)
            st = K.ProdigyState(p, d0=1e-3)
            if misaligned:
                st.p0, st.exp_avg, st.exp_avg_sq, st.s = (view(t) for t in (st.p0, st.exp_avg, st.exp_avg_sq, st.s))
            for i, gr in enumerate(grads):
                lr = (0.25, 0.5, 1.0)[i]
                K.prodigy_step(p, gr, st, _word(cuda, lr) if form == "word" else lr, (0.9, 0.99), EPS, WD,
                               grad_scale=0.5, amp_state=None if sc is None else sc.state, **hyp)
            assert st.scalars()["k"] == 3 and st.scalars()["updated"] == 1 and not torch.equal(p.cpu(), p0)
            runs.append([t.cpu().contiguous().view(torch.uint8).numpy().tobytes()
                         for t in (p, st.exp_avg, st.exp_avg_sq, st.s, st.state)])
        assert runs[0] == runs[1], amp


# ----------------------------------------------------------------------------------------------------------------------
# 3. the trainers
# ----------------------------------------------------------------------------------------------------------------------
def _unet(cuda):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    return unet


def _fill_grad(unet, step):
    """Fixed random values into the flat gradient (3 x N(0, 1): the norm clips)."""
    unet.lora.grad.copy_(torch.randn(unet.lora.grad.shape, device=unet.lora.grad.device, generator=_gen(50 + step)) * 3)


@pytest.mark.parametrize("adam8", [False, True])
def test_trainer_follows_the_schedule(cuda, adam8):
    """linear, w = 2, T = 6, seven optimizer steps: lambda = 0, 1/2, 1, 3/4, 1/2, 1/4, 0."""
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, trainable_segments
    unet = _unet(cuda)
    kw = dict(lr=1e-3, weight_decay=1e-2, use_8bit_adam=adam8)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, lr_scheduler="linear", lr_warmup_steps=2, max_train_steps=6, **kw)
    sched = tr.lr_schedule
    assert sched is not None and tr.lr == 1e-3 and tr.last_lr is None
    master = unet.lora.master
    mirror = master.clone()
    if adam8:
        st8 = K.Adam8State(master.numel(), cuda, segments=trainable_segments(unet))
        work = torch.zeros_like(unet.lora.work)
    else:
        m, v = torch.zeros_like(master), torch.zeros_like(master)
        # CPU torch.optim.AdamW + the transformers scheduler, stepped the way the script does (DB:1959-1963)
        from transformers.optimization import get_scheduler
        p_ref = master.detach().cpu().clone().requires_grad_(True)
        opt = torch.optim.AdamW([p_ref], lr=1e-3, betas=tr.betas, eps=tr.adam_eps, weight_decay=1e-2)
        sch = get_scheduler("linear", opt, num_warmup_steps=2, num_training_steps=6)
    lam = [0.0, 0.5, 1.0, 0.75, 0.5, 0.25, 0.0]
    clip = torch.zeros(2, device=cuda)
    for step in range(1, 8):
        _fill_grad(unet, step)
        grad = unet.lora.grad.clone()
        before = master.clone()
        tr.optimizer_step()
        lr32 = np.float32(sched.lr(step - 1))
        assert tr.opt_step == step and tr.last_lr == float(lr32) == float(np.float32(1e-3 * lam[step - 1]))
        K.grad_clip_coef(grad, tr.max_grad_norm, out=clip)
        assert clip[1].item() < 1.0
        if adam8:
            K.adamw8bit_step(mirror, grad, st8, float(lr32), tr.betas, tr.adam_eps, tr.wd, step, clip=clip,
                             out_bf16=work, zero_grad=True)
            for (k, a), b in zip(tr.adam8.tensors().items(), st8.tensors().values()):
                assert torch.equal(a, b), (step, k)
        else:
            K.adamw_step(mirror, grad, m, v, float(lr32), tr.betas, tr.adam_eps, tr.wd, step, clip=clip)
            assert torch.equal(_bits(tr.exp_avg), _bits(m)) and torch.equal(_bits(tr.exp_avg_sq), _bits(v))
            p_ref.grad = grad.cpu()
            torch.nn.utils.clip_grad_norm_([p_ref], tr.max_grad_norm)
            assert abs(opt.param_groups[0]["lr"] - 1e-3 * lam[step - 1]) < 1e-15
            opt.step()
            sch.step()
        assert torch.equal(_bits(master), _bits(mirror)), step
        if step in (1, 7):  # lambda = 0: before the ramp and past T the master does not move
            assert torch.equal(_bits(master), _bits(before))
        else:
            assert not torch.equal(master, before)
        assert unet.lora.grad.abs().max().item() == 0.0
    if not adam8:
        d = (master.cpu() - p_ref.detach()).abs().max().item()
        print(f"  trainer vs CPU torch.optim.AdamW + transformers linear schedule: max |diff| {d:.2e}")
        assert d < 1e-5


def test_constant_schedule_runs_the_fixed_rate_step(cuda):
    """lr_scheduler="constant" (with any warm-up) builds nothing: no schedule object, no lr word, last_lr = lr."""
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _unet(cuda)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, lr=1e-3, lr_scheduler="constant", lr_warmup_steps=500)
    assert tr.lr_schedule is None and tr.lr_word is None
    mirror = unet.lora.master.clone()
    m, v = torch.zeros_like(mirror), torch.zeros_like(mirror)
    _fill_grad(unet, 1)
    grad = unet.lora.grad.clone()
    tr.optimizer_step()
    K.adamw_step(mirror, grad, m, v, 1e-3, tr.betas, tr.adam_eps, tr.wd, 1, clip=K.grad_clip_coef(grad, 1.0))
    assert torch.equal(_bits(unet.lora.master), _bits(mirror)) and tr.last_lr == 1e-3


def test_prodigy_warms_up_from_zero(cuda, capsys):
    """Prodigy with constant_with_warmup, w = 2, no safeguard warm-up: lr = 0, 1/2, 1, 1.  Step 1 runs at lr = 0 --
    which the host-argument entry rejects -- and follows the restatement with dlr = 0: s stays 0, the denominator is
    0, parameters, d and k keep their values and UPDATED = 0, while the schedule itself advances.  The later steps
    against tests/prodigy_ref.py with its lr set per step, at the bounds of tests/test_gpu_prodigy.py (1e-5)."""
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _unet(cuda)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, optimizer="prodigy", lr=1.0, weight_decay=1e-2,
                    lr_scheduler="constant_with_warmup", lr_warmup_steps=2, prodigy_d0=1e-3, prodigy_d_coef=4.0,
                    betas=(0.9, 0.99))
    o = tr.prodigy_opts
    assert not o["safeguard_warmup"]
    master = unet.lora.master
    r = ProdigyRef(master.cpu().numpy(), lr=1.0, betas=tr.betas, beta3=o["beta3"], eps=tr.adam_eps,
                   weight_decay=tr.wd, decouple=o["decouple"], use_bias_correction=o["use_bias_correction"],
                   safeguard_warmup=False, d0=1e-3, d_coef=4.0, growth_rate=o["growth_rate"])
    c = torch.randn(master.shape, device=cuda, generator=_gen(70))
    want_lr = [0.0, 0.5, 1.0, 1.0]
    for step in range(1, 5):
        grad = c + 0.3 * torch.randn(master.shape, device=cuda, generator=_gen(70 + step))
        unet.lora.grad.copy_(grad)
        before = master.clone()
        tr.optimizer_step()
        assert tr.opt_step == step and tr.last_lr == want_lr[step - 1] == tr.lr_word.item()
        r.lr = np.float32(want_lr[step - 1])
        r.step(grad.cpu().numpy(), np.float32(1.0) * np.float32(tr.clip_buf[1].item()))
        sc = tr.prodigy.scalars()
        if step == 1:
            assert torch.equal(_bits(master), _bits(before))
            assert (sc["k"], sc["updated"], sc["d"], sc["d_denom"], sc["dlr"]) == (0, 0, 1e-3, 0.0, 0.0)
            assert tr.prodigy.s.abs().max().item() == 0.0 and tr.prodigy.exp_avg.abs().max().item() > 0.0
            assert (r.k, r.updated, r.d) == (0, 0, 1e-3)
            continue
        assert sc["k"] == r.k == step - 1 and sc["updated"] == 1  # the schedule counts steps, not Prodigy's k
        ref_move = r.p.astype(np.float64) - r.p0.astype(np.float64)
        move = master.cpu().double().numpy() - tr.prodigy.p0.cpu().double().numpy()
        rel = {"p-p0": np.abs(move - ref_move).max() / np.abs(ref_move).max()}
        for k, got, want in (("m", tr.prodigy.exp_avg, r.m), ("v", tr.prodigy.exp_avg_sq, r.v), ("s", tr.prodigy.s, r.s)):
            rel[k] = np.abs(got.cpu().double().numpy() - want.astype(np.float64)).max() / np.abs(want).max()
        for k in ("d", "d_max", "d_numerator"):
            rel[k] = abs(sc[k] - getattr(r, k)) / abs(getattr(r, k)) if getattr(r, k) else abs(sc[k])
        with capsys.disabled():
            print(f"\n  [prodigy warm-up step {step} lr {want_lr[step - 1]}] d/d0 {sc['d'] / sc['d0']:.4g}  " +
                  "  ".join(f"{k} {e:.2e}" for k, e in rel.items()))
        assert np.abs(ref_move).max() > 0
        for k, e in rel.items():
            assert e <= 1e-5, (step, k, e)
