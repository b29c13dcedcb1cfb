"""Randomised parity of the fused step log-prob / pairwise loss kernels (csrc/pso_loss.hip) against the numpy oracle
(oracle/pso_math.py), at the shapes where the reduction, the per-image coefficients, the pair loops and the clamp
branches can go wrong: more than one LP_CHUNK = 8192 chunk, a ragged last chunk, mixed timesteps inside every pair,
up to 1024 pairs, members on both sides of the clamp and (0, 0) ties.

One seeded numpy builder (`build_case`) makes every input; the CPU test at the end checks the builder's own
conditions with the oracle alone, the GPU tests compare the kernels with the same oracle values.  The 16-bit element
type comes from `compute_dtype()`, so the module runs unchanged under the fp16 library (PSO_LIB=f16 child of
tests/test_f16_build.py).

Timesteps.  DMD2 images cycle through (t, t_prev) = (999,749), (749,499), (499,249), (249,0).  Turbo images cycle
through t = 999, 749, 499 of the 4-step table: its last step t = 249 has sigma_up = 0 (sigma_to = 0, the
deterministic step the trainer never trains, T:218-221), so its log-prob is -log 0 and no case can hold it.  The
bf16 replay mode leaves out (249, 0) for the same reason: alphas_cumprod[0] = 0.99915 is 1.0 in bf16, so the
reference's own bf16 std sqrt(1 - abar_prev) is 0 there.

Clamp plan.  prev is the oracle's own step from eps_ref, so w = (prev - mean_ref) / std is the drawn noise.  With
eps_pol = eps_ref + delta * r and g = (d mean / d eps) / std, the log-ratio is exactly
    lp_pol - lp_ref = a c1 - a^2 c2 / 2,   a = g delta,  c1 = mean(w r),  c2 = mean(r^2)
(float64, before the element-type rounding of eps).  r = sign(g) w + u / 2 with u standard normal; delta is the
smaller root for the planned log-ratio (inside: +-0.3 log 1.1; above: 2.5 log 1.1; below: 2.5 log 0.9), so the sign of
the move follows the sign of r . (prev - mean).  A positive target needs c1^2 >= 3 c2 target; where a 4-element image
cannot reach it, the member takes the negative target of its kind instead (decided from the inputs, no seed search).
Pair p follows plan[p % 4] = (in, in), (below, above), (above, in), (in, below); a single pair cannot hold all three
situations, so P = 1 cases take (in, below) at n = 4 and (above, in) at n = 1028."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import pso_math

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BETA, CLIP = 50.0, 0.1  # the reference configs' train.beta / train.eps (tests/golden/run_config_*.json)
L_HI, L_LO = float(np.log(1.1)), float(np.log(0.9))
TURBO_T = [999.0, 749.0, 499.0]
DMD_T = [(999, 749), (749, 499), (499, 249), (249, 0)]
PLAN = [(0, 0), (-1, 1), (1, 0), (0, -1)]  # 0 inside, -1 below 1 - clip, +1 above 1 + clip
PREFS = np.array([[1, -1], [-1, 1], [0, 0]], np.float32)
LATENT = {"dmd_f16": "fp16", "dmd_bf16": "bf16"}
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}

SHAPES = [(8192, 2),    # one exact chunk
          (8196, 2),    # second chunk of 4 elements (one active thread)
          (17412, 3),   # three chunks, the last ragged against the 1024-element thread stride
          (4, 300),     # the finalize loops take a second trip
          (4, 1024),    # ... and a last one
          (4, 1), (1028, 1)]  # below one thread row
CASES = [(m, n, P) for m in ("turbo", "dmd") for n, P in SHAPES] + \
        [(m, n, P) for m in ("dmd_f16", "dmd_bf16") for n, P in [(8196, 2), (17412, 3)]]
CASE_IDS = [f"{m}-n{n}-P{P}" for m, n, P in CASES]


def _tables():
    t = np.load(os.path.join(GOLD, "pso_turbo_N4_P2_h16_s0_seed4.npz"))
    d = np.load(os.path.join(GOLD, "pso_dmd_P2_h16_t749_seed11.npz"))
    return t["sigmas"], t["timesteps"], d["alphas_cumprod"]


def round_elem(a, elem):
    """float32 values rounded to a torch 16-bit dtype (the library's element type), as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(elem).float().numpy()


def oracle_lp(c, eps, prev=None, noise=None):
    """(prev, lp) of case c's step by the oracle, on `eps` [B, n]."""
    if c["mode"] == "turbo":
        return pso_math.turbo_step_logprob(c["x"], eps, *c["ocoef"], prev=prev, noise=noise)
    if c["latent"] is None:
        return pso_math.dmd_step_logprob(c["x"], eps, *c["ocoef"], prev=prev, noise=noise)
    sa, sb = c["ocoef"][:2]
    return pso_math.dmd_step_logprob_latent(c["x"], eps, sa, sb, c["ac"], c["t_prev"], c["latent"], prev=prev,
                                            noise=noise)


def step_scalars(c):
    """Per image, float64: std of the step, d mean / d eps, and the log-density denominator 2 std^2 as the kernel's
    coefficient row holds it."""
    if c["mode"] == "turbo":
        s, su, dt = (v.astype(np.float64) for v in c["ocoef"])
        return su, dt, 2.0 * su * su
    sa, sb, sap, sbp = (v.astype(np.float64) for v in c["ocoef"])
    den = 2.0 * sbp * sbp
    if c["latent"] is not None:
        sap, sbp, den, _ = (v.astype(np.float64) for v in pso_math.dmd_coefs_latent(c["ac"], c["t_prev"], c["latent"]))
    return sbp, -sap * sb / sa, den


def mean_of(c, eps):
    """The step's mean by the oracle: its prev for zero noise (x + 0 and the latent-dtype re-rounding are exact)."""
    return oracle_lp(c, eps, noise=np.zeros((1, c["n"]), np.float32))[0]


@functools.lru_cache(maxsize=None)
def build_case(mode, n, P, elem):
    from pairwise_sample_optimization_amd import pso_core
    sigmas, timesteps, ac = _tables()
    B = 2 * P
    latent = LATENT.get(mode)
    rng = np.random.default_rng([("turbo", "dmd", "dmd_f16", "dmd_bf16").index(mode), n, P])
    rnd = (lambda a: pso_math.round_latent(a, latent)) if latent else (lambda a: round_elem(a, elem))
    c = {"mode": mode, "n": n, "P": P, "latent": latent, "ac": ac, "elem_eps": latent is None}
    c["x"] = rng.standard_normal((B, n)).astype(np.float32)
    c["noise"] = rng.standard_normal((B, n)).astype(np.float32)
    if latent:  # latent-valued inputs
        c["x"], c["noise"] = rnd(c["x"]), rnd(c["noise"])
    if mode == "turbo":
        t = np.array([TURBO_T[i % 3] for i in range(B)], np.float32)
        c["ocoef"] = pso_math.turbo_coefs(sigmas, timesteps, t)
        c["coef"] = pso_core.turbo_coef(torch.from_numpy(sigmas), torch.from_numpy(timesteps), torch.from_numpy(t))
    else:
        steps = DMD_T[:3] if latent == "bf16" else DMD_T
        t = np.array([steps[i % len(steps)][0] for i in range(B)], np.int64)
        c["t_prev"] = np.array([steps[i % len(steps)][1] for i in range(B)], np.int64)
        c["ocoef"] = pso_math.dmd_coefs(ac, t, c["t_prev"])
        kw = {"latent_dtype": torch.float16 if latent == "fp16" else torch.bfloat16} if latent else {}
        c["coef"] = pso_core.dmd_coef(torch.from_numpy(ac), torch.from_numpy(t), torch.from_numpy(c["t_prev"]), **kw)
    c["t"] = t
    c["eps_ref"] = rnd(rng.standard_normal((B, n)).astype(np.float32))
    c["prev"], c["lp_ref"] = oracle_lp(c, c["eps_ref"], noise=c["noise"])
    # the clamp plan: delta per image from the exact quadratic of the log-ratio (module docstring)
    std, dmu, _ = step_scalars(c)
    g = dmu / std
    w = (c["prev"].astype(np.float64) - mean_of(c, c["eps_ref"]).astype(np.float64)) / std[:, None]
    r = (np.sign(g)[:, None] * w + 0.5 * rng.standard_normal((B, n))).astype(np.float32)
    c1, c2 = (w * r).mean(1), (r.astype(np.float64) ** 2).mean(1)
    if P == 1:
        plan = np.array([0, -1] if n == 4 else [1, 0])
    else:
        plan = np.array([PLAN[p % 4][k] for p in range(P) for k in range(2)])
    member = np.arange(B) % 2
    tau = np.where(plan == 0, np.where(member == 0, 0.3, -0.3) * L_HI, np.where(plan > 0, 2.5 * L_HI, 2.5 * L_LO))
    short = (tau > 0) & (c1 * c1 < 3.0 * c2 * tau)  # a positive target this image cannot reach
    plan = np.where(short & (plan > 0), -1, plan)
    tau = np.where(short, np.where(plan == 0, -0.3 * L_HI, 2.5 * L_LO), tau)
    sg = np.where(c1 >= 0, 1.0, -1.0)
    a = (c1 - sg * np.sqrt(c1 * c1 - 2.0 * c2 * tau)) / c2
    c["plan"], c["tau"], c["delta"] = plan, tau, a / g
    c["eps_pol"] = rnd(c["eps_ref"] + (c["delta"][:, None] * r).astype(np.float32))
    _, c["lp_pol"] = oracle_lp(c, c["eps_pol"], prev=c["prev"])
    kinds = 2 if mode == "turbo" else 3  # (0, 0) ties are DMD2's (strict Pareto dominance)
    c["pref"] = PREFS[np.arange(P) % kinds].copy()
    return c


def _ratios(c):
    d = pso_math.round_latent((c["lp_pol"] - c["lp_ref"]).astype(np.float32), c["latent"])
    return pso_math.round_latent(np.exp(d).astype(np.float32), c["latent"]).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# GPU side
# ----------------------------------------------------------------------------------------------------------------------
def _mode_id(mode):
    from pairwise_sample_optimization_amd import _lib
    return {"turbo": _lib.MODE_TURBO, "dmd": _lib.MODE_DMD, "dmd_f16": _lib.MODE_DMD_F16,
            "dmd_bf16": _lib.MODE_DMD_BF16}[mode]


def _case(mode, n, P):
    import pairwise_sample_optimization_amd as pkg
    return build_case(mode, n, P, pkg.compute_dtype())


def _dev(c, dev):
    """Device tensors of case c; eps in the library's element type (exact: the values are rounded to it) except in
    the replay modes, whose latent-valued eps stay fp32."""
    import pairwise_sample_optimization_amd as pkg
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: T(c[k]) for k in ("x", "noise", "prev", "eps_ref", "eps_pol", "pref")}
    d["coef"] = c["coef"].to(dev)
    if c["elem_eps"]:
        d["eps_ref32"], d["eps_pol32"] = d["eps_ref"], d["eps_pol"]
        d["eps_ref"], d["eps_pol"] = d["eps_ref"].to(pkg.compute_dtype()), d["eps_pol"].to(pkg.compute_dtype())
        assert torch.equal(d["eps_pol"].float(), d["eps_pol32"])
    return d


def _lp_close(c, got, want):
    np.testing.assert_allclose(got, want, rtol=ULP[c["latent"]] if c["latent"] else 1e-6)


def _prev_close(c, got, want):
    if c["latent"]:
        np.testing.assert_array_equal(got, want)  # the replay modes' element-wise arithmetic is bit-exact
    else:
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)  # the figure of tests/test_gpu_pso_loss.py


@gpu
@pytest.mark.parametrize("mode,n,P", CASES, ids=CASE_IDS)
def test_step_logprob_vs_oracle(cuda, mode, n, P):
    """pso_step_logprob in its three forms on B = 2P images of mixed timesteps: noise per image, one shared [1, n]
    noise, prev given.  prev rtol = atol = 2e-6 (tests/test_gpu_pso_loss.py), lp rtol 1e-6 (the oracle docstring's
    figure for another summation order); replay modes: prev bit-exact, lp one latent ulp."""
    from pairwise_sample_optimization_amd import kernels as K
    c = _case(mode, n, P)
    d = _dev(c, cuda)
    m = _mode_id(mode)
    prev, lp = K.step_logprob(m, d["x"], d["eps_ref"], d["coef"], noise=d["noise"])
    _prev_close(c, prev.cpu().numpy(), c["prev"])
    _lp_close(c, lp.cpu().numpy(), c["lp_ref"])
    rprev, rlp = oracle_lp(c, c["eps_ref"], noise=c["noise"][:1])
    prev, lp = K.step_logprob(m, d["x"], d["eps_ref"], d["coef"], noise=d["noise"][:1].contiguous(),
                              noise_shared=True)
    _prev_close(c, prev.cpu().numpy(), rprev)
    _lp_close(c, lp.cpu().numpy(), rlp)
    prev, lp = K.step_logprob(m, d["x"], d["eps_pol"], d["coef"], prev=d["prev"])
    assert prev is d["prev"]
    _lp_close(c, lp.cpu().numpy(), c["lp_pol"])


@gpu
@pytest.mark.parametrize("mode", ["turbo", "dmd"])
def test_step_logprob_many_images(cuda, mode):
    """B = 130 images of n = 8196: lp_finalize_kernel runs three 64-wide blocks, the last with two live threads."""
    from pairwise_sample_optimization_amd import kernels as K
    c = _case(mode, 8196, 65)
    d = _dev(c, cuda)
    prev, lp = K.step_logprob(_mode_id(mode), d["x"], d["eps_ref"], d["coef"], noise=d["noise"])
    assert lp.shape == (130,)
    _prev_close(c, prev.cpu().numpy(), c["prev"])
    _lp_close(c, lp.cpu().numpy(), c["lp_ref"])


def _ws(K, c, dev):
    """The partials' workspace, every double a NaN: a slot the forward does not write shows in the log-probs."""
    return K.pair_loss_ws(c["P"], c["n"], dev).fill_(0xFF)


def _fwd(K, c, d, ws):
    return K.pair_loss_fwd(_mode_id(c["mode"]), d["x"], d["prev"], d["eps_pol"], d["eps_ref"], d["coef"], d["pref"],
                           BETA, CLIP, ws)


@gpu
@pytest.mark.parametrize("mode,n,P", CASES, ids=CASE_IDS)
def test_pair_loss_fwd_vs_oracle(cuda, mode, n, P, capsys):
    """pso_pair_loss_fwd: the four log-probs of every pair against the oracle's (rows differ in timestep and in
    delta, so an image that read another image's coefficients or partials fails here), then the loss twice.

    Scalar stage alone: pso_math.pair_loss on the kernel's own lp against the kernel's loss, absolute bound
    4 beta 2^-23 = 2.4e-5 (two members, one ulp each of expf and logf at a ratio near 1, |dL/dz| <= 1).
    End to end, against pso_math.pair_loss on the oracle's lp: that bound plus 2 beta 1e-6 max|lp| (the lp tolerance
    carried through beta * log-ratio), max|lp| taken per case from the oracle's log-probs.
    Observed on an MI355X, largest |kernel - oracle| over the shapes of a mode, scalar stage and end to end alike
    (the kernel's lp and the oracle's give the same float32 loss): turbo 2.4e-7, dmd 1.9e-7, dmd_f16 0, dmd_bf16 0
    under the bf16 library."""
    from pairwise_sample_optimization_amd import kernels as K
    c = _case(mode, n, P)
    d = _dev(c, cuda)
    ws = _ws(K, c, cuda)
    loss, lp = _fwd(K, c, d, ws)
    loss2, lp2 = _fwd(K, c, d, ws)
    assert torch.equal(lp, lp2) and torch.equal(loss, loss2)  # fixed-order fp64 partials: same bits every call
    lp = lp.cpu().numpy()
    assert np.isfinite(lp).all()
    _lp_close(c, lp[:, 0], c["lp_pol"])
    _lp_close(c, lp[:, 1], c["lp_ref"])
    kp, kr = lp[:, 0].reshape(P, 2), lp[:, 1].reshape(P, 2)
    stage, _, inside = pso_math.pair_loss(kp, kr, c["pref"], BETA, CLIP, latent=c["latent"])
    np.testing.assert_array_equal(inside.reshape(-1), c["plan"] == 0)
    full, _, _ = pso_math.pair_loss(c["lp_pol"].reshape(P, 2), c["lp_ref"].reshape(P, 2), c["pref"], BETA, CLIP,
                                    latent=c["latent"])
    e_stage, e_full = abs(loss.item() - float(stage)), abs(loss.item() - float(full))
    bound = 4.0 * BETA * 2.0 ** -23
    maxlp = max(np.abs(c["lp_pol"]).max(), np.abs(c["lp_ref"]).max())
    with capsys.disabled():
        print(f"\n  [pair_loss_fwd {mode} n={n} P={P}] loss {loss.item():.6f}  scalar stage {e_stage:.3e} "
              f"(bound {bound:.3e})  end to end {e_full:.3e} (bound {bound + 2.0 * BETA * 1e-6 * maxlp:.3e})")
    assert e_stage <= bound
    assert e_full <= bound + 2.0 * BETA * 1e-6 * maxlp


def _dlp64(c, lp):
    """pso_math.pair_loss_dlp's formula in float64 (the replay modes keep their latent-dtype roundings: those are
    the reference's semantics, not float32 noise)."""
    P = c["P"]
    rl = (lambda v: pso_math.round_latent(v.astype(np.float32), c["latent"]).astype(np.float64)) if c["latent"] \
        else (lambda v: v)
    lp = lp.astype(np.float64)
    r = rl(np.exp(rl(lp[:, 0] - lp[:, 1]))).reshape(P, 2)
    lo, hi = float(np.float32(1) - np.float32(CLIP)), float(np.float32(1) + np.float32(CLIP))
    inside = (r >= lo) & (r <= hi)
    lr = rl(BETA * rl(np.log(rl(np.clip(r, lo, hi)))))
    z = (lr * c["pref"]).sum(1)
    one_minus_sig = 1.0 / (1.0 + np.exp(z))
    return (-one_minus_sig[:, None] * BETA * c["pref"] * inside / P).reshape(-1)


def _bwd_reference(c, lp):
    """dL/d eps_pol [2P, n] for an upstream gradient of 1, twice: (a) the float32 oracle, pso_math.pair_loss_dlp on
    the kernel's own log-probs (the backward kernel re-derives exactly those from the same partials) times
    dlp_deps_turbo / dlp_deps_dmd; (b) the same formulas in float64."""
    P, n = c["P"], c["n"]
    dlp = pso_math.pair_loss_dlp(lp[:, 0].reshape(P, 2), lp[:, 1].reshape(P, 2), c["pref"], BETA, CLIP,
                                 latent=c["latent"]).reshape(-1).astype(np.float64)
    std, dmu, den = step_scalars(c)
    x, e, prev = (c[k].astype(np.float64) for k in ("x", "eps_pol", "prev"))
    if c["mode"] == "turbo":
        per = pso_math.dlp_deps_turbo(c["x"], c["eps_pol"], c["prev"], *c["ocoef"])
        mean64 = x + e * dmu[:, None]  # x + ((x - (x - s e)) / s) dt
    elif c["latent"] is None:
        per = pso_math.dlp_deps_dmd(c["x"], c["eps_pol"], c["prev"], *c["ocoef"])
        sa, sb, sap, _ = (v.astype(np.float64)[:, None] for v in c["ocoef"])
        mean64 = sap * ((x - sb * e) / sa)
    else:  # the replay modes' mean is latent-rounded: the same formula on the oracle's latent-dtype mean
        mean64 = mean_of(c, c["eps_pol"]).astype(np.float64)
        per = (prev - mean64) * (2.0 / den * dmu / n)[:, None]
    per64 = (prev - mean64) * (2.0 / den * dmu / n)[:, None]
    return dlp[:, None] * per.astype(np.float64), _dlp64(c, lp)[:, None] * per64


@gpu
@pytest.mark.parametrize("mode,n,P", CASES, ids=CASE_IDS)
def test_pair_loss_bwd_vs_oracle(cuda, mode, n, P, capsys):
    """pso_pair_loss_bwd, fp32 output, grad_out = 2.0 on device, grad_scale = 0.5: largest absolute difference per
    member <= 2e-5 max|ref| + 1e-12 (the bound of tests/test_gpu_pso_loss.py, its measured t = 999 amplification
    included); rows of a member outside the clamp and both rows of a (0, 0) pair are zero in every element.
    Then the options: grad_out=None, fp32 eps_pol, the element-type output (the one the trainer uses) and the
    element-type output under the loss scaler's initial scale 65536.

    Floor of the bound.  The gradient's scalar is (1 - sigmoid(z)) in float32, in the kernel as in the oracle and in
    the reference's -log(sigmoid(z)) autograd: one ulp of sigmoid(z) near 1 (6e-8) is 6e-8 / (1 - sigmoid(z)) of the
    whole row, and no element-wise bound holds it.  Where one pair decides max|ref| (P = 1, one member outside the
    clamp, z = 6.7, 1 - sigmoid = 1.2e-3) 2e-5 cannot be met by any float32 evaluation: dmd n = 4 P = 1 measured
    kernel - oracle 9.27e-5 of max|ref| while the float32 oracle itself stands 5.05e-5 from the same formulas in
    float64 (the kernel 4.22e-5).  So the bound has the floor 2 |oracle - float64|, computed per case; it exceeds
    2e-5 only in the four P = 1 cases (turbo 4.3e-5 and 4.0e-5, dmd 1.01e-4 and 2.6e-5).  Everywhere else observed
    kernel - oracle <= 6.6e-6 of max|ref| (dmd n = 8196 P = 2), replay modes <= 1.5e-7."""
    import pairwise_sample_optimization_amd as pkg
    from pairwise_sample_optimization_amd import kernels as K
    c = _case(mode, n, P)
    d = _dev(c, cuda)
    m = _mode_id(mode)
    elem = pkg.compute_dtype()
    ws = _ws(K, c, cuda)
    _, lp = _fwd(K, c, d, ws)
    bwd = lambda eps=d["eps_pol"], **kw: K.pair_loss_bwd(m, d["x"], d["prev"], eps, d["coef"], d["pref"], BETA, CLIP,
                                                         ws, **kw)
    go = torch.full((), 2.0, device=cuda)
    g32 = bwd(grad_out=go, grad_scale=0.5, out_dtype=torch.float32)
    assert torch.equal(g32, bwd(grad_out=go, grad_scale=0.5, out_dtype=torch.float32))  # deterministic
    g = g32.cpu().numpy().astype(np.float64)
    ref, ref64 = _bwd_reference(c, lp.cpu().numpy())
    zero = (c["plan"] != 0) | np.repeat((c["pref"] == 0).all(1), 2)
    assert zero.any() and not zero.all()
    assert (g[zero] == 0).all() and (ref[zero] == 0).all()
    assert (np.abs(g[~zero]).max(1) > 0).all()
    fails = []
    for k in range(2):
        scale = max(np.abs(ref[k::2]).max(), 1e-30)
        err = np.abs(g[k::2] - ref[k::2]).max()
        floor = 2.0 * np.abs(ref[k::2] - ref64[k::2]).max()
        err64 = np.abs(g[k::2] - ref64[k::2]).max()
        with capsys.disabled():
            print(f"\n  [pair_loss_bwd {mode} n={n} P={P} member {k}] max|ref| {scale:.3e}  kernel - oracle {err:.3e} "
                  f"({err / scale:.2e} of max; bound 2e-5)  2 |oracle - float64| {floor:.3e} ({floor / scale:.2e})  "
                  f"kernel - float64 {err64:.3e} ({err64 / scale:.2e})")
        if err > max(2e-5 * scale, floor) + 1e-12:
            fails.append((k, err, scale, floor))
    assert not fails, fails
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    # grad_out=None means an upstream gradient of 1: 1 * 1.0 and 2 * 0.5 are the same float
    assert torch.equal(bits(bwd(grad_scale=1.0, out_dtype=torch.float32)), bits(g32))
    if c["elem_eps"]:  # fp32 eps_pol holding the same values: same bits
        assert torch.equal(bits(bwd(d["eps_pol32"], grad_out=go, grad_scale=0.5, out_dtype=torch.float32)), bits(g32))
    # element-type output: the same arithmetic, only the store differs
    assert torch.equal(bits(bwd(grad_out=go, grad_scale=0.5, out_dtype=elem)), bits(g32.to(elem)))
    gs32 = bwd(grad_scale=65536.0, out_dtype=torch.float32)
    gs = bwd(grad_scale=65536.0)  # out_dtype defaults to the element type
    assert gs.dtype == elem
    assert torch.equal(bits(gs), bits(gs32.to(elem)))  # equal, and the same inf where the cast overflows
    assert not torch.isnan(gs.float()).any()


@gpu
@pytest.mark.parametrize("mode", ["turbo", "dmd"])
@pytest.mark.parametrize("P", [300, 1024])
def test_pair_loss_from_lp_many_pairs(cuda, mode, P):
    """pso_pair_loss_from_lp where its 256-thread loop takes a second and a last trip, on random log-probs with
    members on both sides of the clamp: loss rtol 2e-6, dlp rtol 2e-5 / atol 1e-9 (the figures of
    tests/test_gpu_reference_fixtures.py)."""
    from pairwise_sample_optimization_amd import kernels as K
    rng = np.random.default_rng(P)
    lp_ref = rng.standard_normal((P, 2)).astype(np.float32)
    tau = rng.choice([0.3 * L_HI, -0.3 * L_HI, 2.5 * L_HI, 2.5 * L_LO], size=(P, 2))
    lp_pol = (lp_ref + tau).astype(np.float32)
    pref = PREFS[rng.integers(0, 2 if mode == "turbo" else 3, size=P)].copy()
    T = lambda a: torch.from_numpy(a).to(cuda)
    loss, dlp = K.pair_loss_from_lp(_mode_id(mode), T(lp_pol), T(lp_ref), T(pref), BETA, CLIP)
    rloss, _, inside = pso_math.pair_loss(lp_pol, lp_ref, pref, BETA, CLIP)
    assert inside.any() and not inside.all()
    np.testing.assert_allclose(loss.item(), rloss, rtol=2e-6)
    g = dlp.cpu().numpy()
    np.testing.assert_allclose(g, pso_math.pair_loss_dlp(lp_pol, lp_ref, pref, BETA, CLIP), rtol=2e-5, atol=1e-9)
    assert (g[~inside] == 0).all()


@gpu
def test_pair_loss_from_lp_rejects_more_than_1024_pairs(cuda):
    from pairwise_sample_optimization_amd import kernels as K, _lib
    z = torch.zeros((1025, 2), device=cuda)
    with pytest.raises(_lib.PsoLibError):
        K.pair_loss_from_lp(_lib.MODE_TURBO, z, z, z, BETA, CLIP)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the builder's own conditions, by the oracle alone (no GPU)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode,n,P", CASES + [("turbo", 8196, 65), ("dmd", 8196, 65)],
                         ids=CASE_IDS + ["turbo-n8196-P65", "dmd-n8196-P65"])
def test_cases_hold_their_conditions(mode, n, P, elem):
    """Every ratio exp(lp_pol - lp_ref) is at least 1e-3 (relative) away from both clamp bounds, so a 1e-6 summation
    difference cannot move a member across a branch; every member is on the side its plan says; inside, below and
    above are all present (P = 1: one inside, one outside member); no pair has equal coefficient rows."""
    c = build_case(mode, n, P, elem)
    assert np.isfinite(c["lp_pol"]).all() and np.isfinite(c["lp_ref"]).all() and np.isfinite(c["eps_pol"]).all()
    r = _ratios(c)
    lo, hi = float(np.float32(1) - np.float32(CLIP)), float(np.float32(1) + np.float32(CLIP))
    assert (np.abs(r - lo) >= 1e-3 * lo).all() and (np.abs(r - hi) >= 1e-3 * hi).all()
    side = np.where(r < lo, -1, np.where(r > hi, 1, 0))
    np.testing.assert_array_equal(side, c["plan"])
    pairs = side.reshape(P, 2)
    if P == 1:
        assert sorted(np.abs(pairs[0])) == [0, 1]
    else:
        assert (pairs == 0).all(1).any() and (side < 0).any() and (side > 0).any()
    coef = c["coef"].numpy().reshape(P, 2, -1)
    assert (coef[:, 0] != coef[:, 1]).any(1).all()
    assert c["coef"].shape == (2 * P, 8)
    if mode != "turbo":
        assert (c["pref"] == 0).all(1).any() or P < 3
