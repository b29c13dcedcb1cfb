"""GPU tests of the Prodigy step (csrc/prodigy.hip, pso_prodigy_step) against the numpy restatement
tests/prodigy_ref.py, and of the trainers and the checkpoint that run on it.

Sizes: fewer elements than one 16-byte vector (3), a ragged tail (1027), more than one workgroup, and more elements than
the 2048 x 256 threads of the capped grid -- a second grid-stride trip on the scalar path (GRID + 3 on 4-byte-misaligned
buffers, `buf[1:]`) and on the vector path (4 (GRID + 3) + 3 on aligned ones).

Inputs of the parity runs: parameters 1e-2 N(0, 1), gradient g_t = c + 0.3 noise_t with a fixed c ~ N(0, 1), d0 = 1e-3,
lr = 1, weight decay 1e-2, eight steps.  betas = (0.9, 0.99) and d_coef = 4 were chosen on the restatement alone so
that d grows by more than 10 x in every case: at prodigyopt's defaults (0.999, d_coef 1) the bias-corrected cases grow
by 1 x (with safeguard) and 6.6 x (without) in eight steps.  The run asserts what makes it non-vacuous: that growth,
|num| >= 0.1 of the sum of the absolute values of its terms at every step (no cancellation in d_hat), and a parameter
movement of at least 1e3 tolerances.

Bounds: m, v, s and p - p0 within 1e-5 max|ref|; d, d_max and d_numerator within rtol 1e-5.  The element products are
float32 in the same order on both sides and the sums are float64, so kernel and restatement differ only where a scalar
(d (1 - b1), d^2 (1 - b2), (d / d0) x, dlr, d eps: a few float32 roundings of 6e-8 each, from float64 values that
differ in the last bits through the summation order and the device's pow) rounds the other way; that is fed back
through eight steps and amplified by at most 10 under the cancellation condition: < 1e-5.
Observed on an MI355X, largest over all 72 parity cases: m, v, s and p - p0 bit-identical to the restatement (0); d and
d_max 4.5e-14, d_numerator 4.5e-14 (no scalar rounded the other way in these runs).  Trainer cases: the same, the
scalars within 4e-16."""
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from prodigy_ref import ProdigyRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 2048 * 256  # threads of the capped grid (prodigy_blocks() in csrc/prodigy.hip)
SIZES = [3, 1027, GRID + 3, 4 * (GRID + 3) + 3]
F32 = np.float32
BETAS, D_COEF, D0, WD, EPS, STEPS = (0.9, 0.99), 4.0, 1e-3, 1e-2, 1e-8, 8
TOL = 1e-5


def _view(x, misaligned, dev):
    """x as a length-n device view: 256-byte aligned, or 4 bytes past it."""
    n = x.numel()
    buf = torch.empty(n + 1, device=dev)
    view = buf[1:] if misaligned else buf[:n]
    view.copy_(x)
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return view


def _state(K, p, misaligned, dev, d0=D0):
    st = K.ProdigyState(p, d0=d0)
    if misaligned:
        st.p0, st.exp_avg, st.exp_avg_sq, st.s = (_view(t, True, dev) for t in (st.p0, st.exp_avg, st.exp_avg_sq, st.s))
    return st


def _inputs(n):
    gen = torch.Generator().manual_seed(n)
    p = 1e-2 * torch.randn(n, generator=gen)
    c = torch.randn(n, generator=gen)
    return gen, p, c


def _run(K, dev, n, misaligned, decouple, bias, safeguard, clipped, ref=True):
    """Eight steps on the device and (ref) in the restatement; returns (p, state, restatement, conditions)."""
    gen, p0, c = _inputs(n)
    p = _view(p0, misaligned, dev)
    st = _state(K, p, misaligned, dev)
    hyp = dict(decouple=decouple, use_bias_correction=bias, safeguard_warmup=safeguard, d_coef=D_COEF)
    r = ProdigyRef(p0.numpy(), lr=1.0, betas=BETAS, eps=EPS, weight_decay=WD, d0=D0, **hyp) if ref else None
    gs = 0.25 if clipped else 1.0
    cancel = []
    for _ in range(STEPS):
        g = c + 0.3 * torch.randn(n, generator=gen)
        gd = _view(g, misaligned, dev)
        clip = K.grad_clip_coef(gd, 1.0, grad_scale=gs) if clipped else None
        K.prodigy_step(p, gd, st, 1.0, BETAS, EPS, WD, grad_scale=gs, clip=clip, **hyp)
        if ref:
            gmul = F32(gs) * F32(clip[1].item()) if clipped else F32(1.0)
            if clipped and n >= 4:
                assert clip[1].item() < 1.0
            r.step(g.numpy(), gmul)
            cancel.append((abs(r.num_last), r.num_abs_terms))
    return p, st, r, cancel


CASES = list(itertools.product([True, False], repeat=4))
MISALIGNED_CASES = [(True, True, True, True), (False, False, False, False)]


def _id(case):
    d, b, s, c = case
    return "-".join(("decoupled" if d else "coupled", "bias" if b else "nobias", "safeguard" if s else "nosafeguard",
                     "clip0.25" if c else "noclip"))


def _check_against_ref(cuda, n, misaligned, case, capsys):
    from pairwise_sample_optimization_amd import kernels as K
    p, st, r, cancel = _run(K, cuda, n, misaligned, *case)
    # the conditions on the inputs, from the restatement alone
    assert r.k == STEPS and r.d >= 10.0 * r.d0, (r.k, r.d / r.d0)
    for num, terms in cancel:
        assert num >= 0.1 * terms, (num, terms)
    ref_move = r.p.astype(np.float64) - r.p0.astype(np.float64)
    assert np.abs(ref_move).max() >= 1e3 * TOL * np.abs(ref_move).max()
    assert np.abs(ref_move).max() >= 1e3 * TOL * np.abs(r.p).max()  # the parameters moved by over 1 % of their scale
    sc = st.scalars()
    got = {"m": st.exp_avg, "v": st.exp_avg_sq, "s": st.s}
    want = {"m": r.m, "v": r.v, "s": r.s}
    rel = {k: np.abs(got[k].cpu().double().numpy() - want[k].astype(np.float64)).max() / np.abs(want[k]).max()
           for k in got}
    move = p.cpu().double().numpy() - st.p0.cpu().double().numpy()
    rel["p-p0"] = np.abs(move - ref_move).max() / np.abs(ref_move).max()
    assert st.p0.cpu().numpy().tobytes() == r.p0.tobytes()
    srel = {k: abs(sc[k] - getattr(r, k)) / abs(getattr(r, k)) for k in ("d", "d_max", "d_numerator")}
    with capsys.disabled():
        print(f"\n  [prodigy n={n} {'misaligned' if misaligned else 'aligned'} {_id(case)}] d/d0 {r.d / r.d0:.3g}  "
              "max|diff| / max|ref|: " + "  ".join(f"{k} {e:.2e}" for k, e in rel.items()) + "  rel: " +
              "  ".join(f"{k} {e:.2e}" for k, e in srel.items()))
    assert (sc["k"], sc["updated"], sc["skipped"]) == (STEPS, 1, 0)
    for k, e in {**rel, **srel}.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("n", SIZES)
def test_prodigy_step_vs_restatement(cuda, n, case, capsys):
    _check_against_ref(cuda, n, False, case, capsys)


@pytest.mark.parametrize("case", MISALIGNED_CASES, ids=_id)
@pytest.mark.parametrize("n", SIZES)
def test_prodigy_step_vs_restatement_misaligned(cuda, n, case, capsys):
    """Every buffer 4 bytes past a 16-byte boundary: the scalar path of both passes (at GRID + 3 its second trip)."""
    _check_against_ref(cuda, n, True, case, capsys)


def _bytes(*ts):
    return [t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts]


@pytest.mark.parametrize("n", [1027, SIZES[-1]])
def test_run_to_run_bits(cuda, n):
    """The same eight steps twice from the same start: p, m, v, s and the state block are the same bytes (the partial
    sums are reduced in a fixed order, no float atomics)."""
    from pairwise_sample_optimization_amd import kernels as K
    runs = []
    for _ in range(2):
        p, st, _, _ = _run(K, cuda, n, False, True, True, True, True, ref=False)
        runs.append(_bytes(p, st.exp_avg, st.exp_avg_sq, st.s, st.state))
    assert runs[0] == runs[1]
    assert K.ProdigyState(p).scalars()["k"] == 0 and st.scalars()["k"] == STEPS


def test_all_zero_gradient(cuda):
    """den = sum|s| = 0: p is bit-identical, d and k unchanged, m decayed by beta1 (pass 1 ran, pass 2 did not)."""
    from pairwise_sample_optimization_amd import kernels as K
    n = 1027
    gen, p0, c = _inputs(n)
    p = p0.to(cuda)
    st = K.ProdigyState(p, d0=D0)
    for _ in range(2):
        K.prodigy_step(p, (c + 0.3 * torch.randn(n, generator=gen)).to(cuda), st, 1.0, BETAS, EPS, WD)
    st.s.zero_()
    before, m0 = st.scalars(), st.exp_avg.cpu().clone()
    pb = _bytes(p)
    assert before["k"] == 2 and before["updated"] == 1 and m0.abs().max() > 0
    K.prodigy_step(p, torch.zeros(n, device=cuda), st, 1.0, BETAS, EPS, WD)
    after = st.scalars()
    assert _bytes(p) == pb
    assert after["updated"] == 0 and after["d_denom"] == 0.0
    for k in ("d", "d_max", "d_numerator", "k", "d0", "skipped"):
        assert after[k] == before[k], k
    assert _bytes(st.exp_avg) == _bytes(torch.tensor(BETAS[0], dtype=torch.float32) * m0)
    fresh_p = p0.to(cuda)
    fresh = K.ProdigyState(fresh_p, d0=D0)  # and from a fresh state
    K.prodigy_step(fresh_p, torch.zeros(n, device=cuda), fresh, 1.0, BETAS, EPS, WD)
    sc = fresh.scalars()
    assert (sc["k"], sc["d"], sc["updated"]) == (0, D0, 0) and _bytes(fresh_p) == _bytes(p0)


def test_found_inf_skips_and_amp_factor_matches(cuda):
    """The loss scaler's found-inf word set by a host-side fill (no non-finite arithmetic on the device): every buffer
    and the Prodigy block keep their bytes except the skipped-step count.  With the word clear the step is the non-amp
    call with grad_scale = GRAD_MUL * CLIP_COEF, bit for bit."""
    from pairwise_sample_optimization_amd import _lib, kernels as K
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    n = SIZES[2]
    gen, p0, c = _inputs(n)
    gmul, coef = F32(0.125), F32(0.37)
    sc = DeviceLossScaler(init_scale=8.0, device=cuda)
    host = sc.state.cpu()
    host.view(torch.float32)[_lib.AMP_GRAD_MUL] = float(gmul)
    host.view(torch.float32)[_lib.AMP_CLIP_COEF] = float(coef)
    hyp = dict(use_bias_correction=True, safeguard_warmup=True, d_coef=D_COEF)
    pa, pb = p0.to(cuda), p0.to(cuda)
    sa, sb = K.ProdigyState(pa, d0=D0), K.ProdigyState(pb, d0=D0)
    grads = [(c + 0.3 * torch.randn(n, generator=gen)).to(cuda) for _ in range(3)]
    for step, g in enumerate(grads):
        if step == 1:  # one skipped step in the middle of the amp run
            host[_lib.AMP_FOUND_INF] = 1
            sc.state.copy_(host)
            keep = _bytes(pa, sa.p0, sa.exp_avg, sa.exp_avg_sq, sa.s, g)
            block = sa.state.cpu().clone()
            K.prodigy_step(pa, g, sa, 1.0, BETAS, EPS, WD, amp_state=sc.state, **hyp)
            assert _bytes(pa, sa.p0, sa.exp_avg, sa.exp_avg_sq, sa.s, g) == keep
            now = sa.state.cpu()
            assert sa.scalars()["skipped"] == 1 and block[_lib.PRODIGY_I32["skipped"]] == 0
            now[_lib.PRODIGY_I32["skipped"]] = 0
            assert torch.equal(now, block)
        host[_lib.AMP_FOUND_INF] = 0
        sc.state.copy_(host)
        K.prodigy_step(pa, g, sa, 1.0, BETAS, EPS, WD, amp_state=sc.state, grad_scale=123.0, **hyp)  # grad_scale unread
        K.prodigy_step(pb, g, sb, 1.0, BETAS, EPS, WD, grad_scale=float(gmul * coef), **hyp)
    assert sb.scalars()["k"] == 3 and sb.scalars()["d"] > D0
    assert _bytes(pa, sa.exp_avg, sa.exp_avg_sq, sa.s) == _bytes(pb, sb.exp_avg, sb.exp_avg_sq, sb.s)
    a, b = sa.state.cpu(), sb.state.cpu()
    a[_lib.PRODIGY_I32["skipped"]] = 0
    assert torch.equal(a, b)
    assert _bytes(sc.state) == _bytes(host)  # the step only reads the scaler's block


def test_argument_errors(cuda):
    from pairwise_sample_optimization_amd import _lib, kernels as K
    p = torch.zeros(8, device=cuda)
    st = K.ProdigyState(p)
    with pytest.raises(_lib.PsoLibError, match="lr"):
        K.prodigy_step(p, p.clone(), st, 0.0, BETAS, EPS, WD)
    e = torch.zeros(0, device=cuda)
    with pytest.raises(_lib.PsoLibError):
        K.prodigy_step(e, e.clone(), K.ProdigyState(e), 1.0, BETAS, EPS, WD)
    l = _lib.lib()
    wsb = l.pso_prodigy_ws_bytes(8)
    ws = torch.empty(wsb, device=cuda, dtype=torch.uint8)
    g = p.clone()

    def raw(ws_bytes):
        return l.pso_prodigy_step(8, p.data_ptr(), g.data_ptr(), st.p0.data_ptr(), st.exp_avg.data_ptr(),
                                  st.exp_avg_sq.data_ptr(), st.s.data_ptr(), st.state.data_ptr(), 1.0, 0.9, 0.99, 0.99,
                                  1e-8, 0.0, 1, 1.0, float("inf"), 1.0, None, None, ws.data_ptr(), ws_bytes,
                                  _lib.stream_ptr())

    with pytest.raises(_lib.PsoLibError, match="workspace"):
        _lib.check(raw(wsb - 1), "pso_prodigy_step")
    _lib.check(raw(wsb), "pso_prodigy_step")
    torch.cuda.synchronize()
    assert st.scalars()["k"] == 0 and st.scalars()["skipped"] == 0  # nothing above moved the state (zero gradient)


# ---- trainers --------------------------------------------------------------------------------------------------------
def _unet(cuda, rank):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=rank, lora_alpha=rank))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    return cfg, unet


def _pso_trainer(cuda, rank, **kw):
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    cfg, unet = _unet(cuda, rank)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, **kw)
    g = torch.Generator(device="cuda").manual_seed(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    tid = compute_time_ids(128, 0, cuda)
    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    sbs = [tr.shuffle(buf, generator=torch.Generator(device="cuda").manual_seed(100 + i)) for i in range(2)]
    return unet, tr, sbs


def _ref_of(tr, master):
    o = tr.prodigy_opts
    return ProdigyRef(master.cpu().numpy(), lr=tr.lr, betas=tr.betas, beta3=o["beta3"], eps=tr.adam_eps,
                      weight_decay=tr.wd, decouple=o["decouple"], use_bias_correction=o["use_bias_correction"],
                      safeguard_warmup=o["safeguard_warmup"], d0=tr.prodigy.scalars()["d0"], d_coef=o["d_coef"],
                      growth_rate=o["growth_rate"])


def _check_trainer_step(tr, unet, r, grad, tag, capsys):
    """After tr.optimizer_step() on `grad` (the trainer's own all-reduced gradient, world 1): the flat master and the
    Prodigy state against the restatement stepped with the trainer's clip coefficient."""
    st = unet.lora
    r.step(grad.cpu().numpy(), F32(1.0) * F32(tr.clip_buf[1].item()))
    sc = tr.prodigy.scalars()
    ref_move = r.p.astype(np.float64) - r.p0.astype(np.float64)
    move = st.master.cpu().double().numpy() - tr.prodigy.p0.cpu().double().numpy()
    rel = {"p-p0": np.abs(move - ref_move).max() / np.abs(ref_move).max()}
    for k, got, want in (("m", tr.prodigy.exp_avg, r.m), ("v", tr.prodigy.exp_avg_sq, r.v), ("s", tr.prodigy.s, r.s)):
        rel[k] = np.abs(got.cpu().double().numpy() - want.astype(np.float64)).max() / np.abs(want).max()
    for k in ("d", "d_max", "d_numerator"):
        rel[k] = abs(sc[k] - getattr(r, k)) / abs(getattr(r, k)) if getattr(r, k) else abs(sc[k])
    with capsys.disabled():
        print(f"\n  [prodigy trainer {tag}] k {sc['k']} d/d0 {sc['d'] / sc['d0']:.4g}  " +
              "  ".join(f"{k} {e:.2e}" for k, e in rel.items()))
    assert np.abs(ref_move).max() > 0 and sc["k"] == r.k and sc["updated"] == 1
    for k, e in rel.items():
        assert e <= TOL, (k, e)
    if st.work.numel() == st.master.numel():  # the working copy is cast(master) ...
        assert torch.equal(st.work.view(torch.int16), st.master.to(st.work.dtype).view(torch.int16))
    else:  # ... or, below rank 8, its zero-padded rank-8 form: a fresh pack of the new master
        w = st.work.clone()
        for name in st.adapter_names():
            A, _ = st.adapter_views(st.master, name)
            Ap, _ = st.adapter_views(w, name, padded=True)
            assert torch.equal(Ap[:st.r], A.to(w.dtype)) and (Ap[st.r:] == 0).all()
        st.refresh()
        assert torch.equal(w, st.work)
    assert st.grad.abs().max().item() == 0.0


@pytest.mark.parametrize("rank", [8, 4])
def test_pso_trainer_steps_match_restatement(cuda, rank, capsys):
    unet, tr, sbs = _pso_trainer(cuda, rank, optimizer="prodigy", lr=1.0)
    assert tr.optimizer == "prodigy" and tr.prodigy is not None
    r = _ref_of(tr, unet.lora.master)
    tr.auto_step = False
    for w, sb in enumerate(sbs):
        tr.train_epoch(sb)
        grad = unet.lora.grad.clone()
        assert grad.abs().max().item() > 0 and torch.isfinite(grad).all()
        tr.optimizer_step()
        _check_trainer_step(tr, unet, r, grad, f"PSO r={rank} window {w + 1}", capsys)
    assert tr.opt_step == 2 and tr.prodigy.scalars()["k"] == 2


def _dreambooth(cuda, **kw):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    from pairwise_sample_optimization_amd.vae import AutoencoderKL, VAEConfig
    cfg, unet = _unet(cuda, 8)
    with torch.device(cuda):
        vae = AutoencoderKL(VAEConfig.tiny())
    vae.init_weights(2)
    g = torch.Generator(device="cuda").manual_seed(4)
    pix = torch.rand(2, 3, 128, 128, device=cuda, generator=g) * 2 - 1
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    return SimpleNamespace(unet=unet, vae=vae, pix=pix, enc=enc, pooled=pooled, tid=compute_time_ids(128, 0, cuda),
                           make=lambda **k: DreamBoothPSOTrainer(unet, vae, **dict(kw, **k)))


def test_dreambooth_trainer_step_matches_restatement(cuda, capsys):
    c = _dreambooth(cuda)
    tr = c.make(loss_type="pso_db", beta_pso=5.0, gradient_accumulation_steps=1, optimizer="prodigy",
                learning_rate=1.0)
    r = _ref_of(tr, c.unet.lora.master)
    tr.auto_step = False
    tr.micro_step(c.pix, c.enc, c.pooled, c.tid, generator=torch.Generator(device="cuda").manual_seed(11))
    grad = c.unet.lora.grad.clone()
    assert grad.abs().max().item() > 0
    tr.optimizer_step()
    _check_trainer_step(tr, c.unet, r, grad, "DreamBooth window 1", capsys)
    assert tr.opt_step == 1


def test_dreambooth_from_args_trains_with_prodigy(cuda):
    """--optimizer prodigy from the script's namespace: refused by default as before, trained with allow_prodigy=True."""
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    c = _dreambooth(cuda)
    args = SimpleNamespace(loss_type="pso_db", beta_pso=5, prior_loss_weight=0.5, optimizer="prodigy",
                           learning_rate=1.0, do_edm_style_training=True, lr_scheduler="constant", lr_warmup_steps=0,
                           gradient_accumulation_steps=1)
    with pytest.raises(ValueError, match="allow_prodigy"):
        DreamBoothPSOTrainer.from_args(c.unet, c.vae, args)
    tr = DreamBoothPSOTrainer.from_args(c.unet, c.vae, args, allow_prodigy=True)
    master0 = c.unet.lora.master.clone()
    tr.micro_step(c.pix, c.enc, c.pooled, c.tid, generator=torch.Generator(device="cuda").manual_seed(11))
    torch.cuda.synchronize()
    sc = tr.prodigy.scalars()
    assert tr.opt_step == 1 and sc["k"] == 1 and sc["updated"] == 1
    assert tr.prodigy_opts["use_bias_correction"] and tr.prodigy_opts["safeguard_warmup"]  # the script's defaults
    assert torch.isfinite(c.unet.lora.master).all() and not torch.equal(c.unet.lora.master, master0)


def test_checkpoint_resume_is_bit_exact(cuda, tmp_path):
    """Save after window 1, load into a fresh Prodigy trainer, run window 2 in both on the same inputs: masters and
    state blocks are the same bytes.  An AdamW trainer refuses the checkpoint."""
    from pairwise_sample_optimization_amd import lora_io
    u1, t1, sbs = _pso_trainer(cuda, 8, optimizer="prodigy", lr=1.0, prodigy_use_bias_correction=True)
    t1.train_epoch(sbs[0])
    assert t1.opt_step == 1
    lora_io.save_state(t1, str(tmp_path))
    u2, t2, _ = _pso_trainer(cuda, 8, optimizer="prodigy", lr=1.0, prodigy_use_bias_correction=True)
    u2.lora.init_gaussian(seed=7, b_std=0.01)  # other weights: everything must come from the checkpoint
    lora_io.load_state(t2, str(tmp_path))
    u2.lora.refresh(cast=True)
    assert _bytes(u1.lora.master, *t1.prodigy.tensors().values()) == _bytes(u2.lora.master,
                                                                             *t2.prodigy.tensors().values())
    assert (t2.opt_step, t2.n_micro) == (t1.opt_step, t1.n_micro)
    for tr in (t1, t2):
        tr.train_epoch(sbs[1])
    torch.cuda.synchronize()
    assert t1.opt_step == t2.opt_step == 2 and t1.prodigy.scalars()["k"] == 2
    assert _bytes(u1.lora.master, t1.prodigy.state) == _bytes(u2.lora.master, t2.prodigy.state)
    assert _bytes(*t1.prodigy.tensors().values()) == _bytes(*t2.prodigy.tensors().values())
    _, t3, _ = _pso_trainer(cuda, 8)
    with pytest.raises(KeyError, match="Prodigy"):
        lora_io.load_state(t3, str(tmp_path))


@pytest.mark.timeout(300)
def test_prodigy_trains_on_the_f16_library(cuda):
    """One window with a DeviceLossScaler under PSO_LIB=f16, in a fresh child process (the element type is per
    process): tests/prodigy_f16_worker_gpu.py."""
    lib = os.path.join(ROOT, "pairwise_sample_optimization_amd", "libpso_amd_f16.so")
    assert os.path.exists(lib), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "prodigy_f16_worker_gpu.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    tail = r.stdout[-4000:] + r.stderr[-4000:]
    assert r.returncode == 0, tail
    assert "PRODIGY_F16_OK k=1" in r.stdout, tail
