"""DoRA on the GPU: the three kernels of csrc/dora.hip against fp64 / bit-exact models with guard bands round every
output, the HIP UNet with DoRA adapters against the fp32 oracle through tests/dora_ref.py's fold, the paired pass, and
one optimizer step of both trainers with a checkpoint round trip."""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

import dora_ref
import parity_util as P

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _vec(n, cuda):
    """A guarded fp32 vector [n] (16-byte aligned) and its guard check."""
    (v,), check = P.guarded(1, [n], dtype=torch.float32, device=cuda)
    return v[0], check


# ----------------------------------------------------------------------------------------------------------------------
# pso_dora_weight_norm
# ----------------------------------------------------------------------------------------------------------------------
# (modules stacked in one base weight, out per module, in, r): the stacked case reads row ranges of one [3 * 64, 128]
# weight as attn1's q / k / v do; r = 4 reads peft's unpadded B [out, 4] rows (16 bytes, any 4-byte boundary)
NORM_CASES = [(1, 64, 64, 8), (3, 64, 128, 8), (1, 1280, 2048, 32), (1, 128, 128, 4)]


@pytest.mark.parametrize("nmod,out,fin,r", NORM_CASES)
def test_weight_norm(cuda, nmod, out, fin, r):
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(out + fin + r)
    s = 0.5 if r == 4 else 1.0
    W = (torch.randn(nmod * out, fin, device=cuda, generator=g) * fin ** -0.5).to(K.ELEM)
    # A and B of all modules back to back in ONE flat fp32 buffer, as the trained master holds them
    flat = torch.empty(nmod * (r * fin + out * r), device=cuda)
    A = flat[:nmod * r * fin].view(nmod * r, fin)
    Bm = flat[nmod * r * fin:].view(nmod * out, r)
    A.copy_(torch.randn(A.shape, device=cuda, generator=g) / r)
    Bm.copy_(torch.randn(Bm.shape, device=cuda, generator=g) * 0.05)
    m, ck_m = _vec(nmod * out, cuda)
    n, ck_n = _vec(nmod * out, cuda)
    gv, ck_g = _vec(nmod * out, cuda)
    sl = lambda v, j, k: v[j * k:(j + 1) * k]
    tab = K.DoraNormTable([(sl(W, j, out), sl(A, j, r), sl(Bm, j, out), s, sl(m, j, out), sl(n, j, out), sl(gv, j, out))
                           for j in range(nmod)], cuda)
    n64 = torch.cat([(sl(W, j, out).double() + s * sl(Bm, j, out).double() @ sl(A, j, r).double()).norm(dim=1)
                     for j in range(nmod)])
    # init mode: m := n, g == 1
    tab.run(init=True)
    torch.cuda.synchronize()
    for ck in (ck_m, ck_n, ck_g):
        ck("pso_dora_weight_norm (init)")
    err = ((n.double() - n64).abs() / n64).max().item()
    print(f"\n  out={nmod}x{out} in={fin} r={r}: max |n - n64| / n64 = {err:.3e}")
    assert err <= 1e-5
    assert torch.equal(_bits(m), _bits(n))
    assert torch.equal(gv, torch.ones_like(gv))
    first = _bits(n).clone()
    # trained magnitudes: g = m / n, n unchanged, identical bits run to run
    m.copy_(n * torch.exp2(torch.rand(n.shape, device=cuda, generator=g) * 2 - 1))
    m0 = m.clone()
    tab.run()
    g1 = _bits(gv).clone()
    tab.run()
    torch.cuda.synchronize()
    for ck in (ck_m, ck_n, ck_g):
        ck("pso_dora_weight_norm")
    assert torch.equal(_bits(n), first) and torch.equal(_bits(gv), g1) and torch.equal(m, m0)
    assert torch.allclose(gv, m0 / n, rtol=3e-7, atol=0)


def test_weight_norm_has_no_cancellation(cuda):
    """B A = -W / s up to a small remainder: the row norm is the remainder's, which a sum |W|^2 + 2 s W.BA + s^2 |BA|^2
    would lose to cancellation.  The kernel squares the summed element, so it keeps the 1e-5 bound."""
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(11)
    out, fin, r = 64, 128, 8
    A = torch.randn(r, fin, device=cuda, generator=g)
    Bm = torch.randn(out, r, device=cuda, generator=g)
    rest = torch.randn(out, fin, device=cuda, generator=g) * 2.0 ** -9
    W = (-(Bm @ A) + rest).to(K.ELEM)
    m, n, gv = (torch.zeros(out, device=cuda) for _ in range(3))
    K.DoraNormTable([(W, A, Bm, 1.0, m, n, gv)], cuda).run(init=True)
    n64 = (W.double() + Bm.double() @ A.double()).norm(dim=1)
    assert (n64 < 0.05 * W.double().norm(dim=1)).all(), "the case must cancel"
    # the products B A are rounded in fp32 before the add: relative to |W| ~ 2^-24 sqrt(r), here ~1e-5 of n
    err = ((n.double() - n64).abs() / n64).max().item()
    print(f"\n  cancelling rows: max |n - n64| / n64 = {err:.3e}")
    assert err <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# pso_dora_scale_fwd / pso_dora_bwd
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(M, N) for N in (64, 192, 1280) for M in (1, 154, 512)]


def _ulp(x, dtype):
    """One unit in the last place of `dtype` at the magnitude of the fp32 values x."""
    bits = 7 if dtype == torch.bfloat16 else 10
    _, e = torch.frexp(x.abs().clamp_min(torch.finfo(dtype).tiny))
    return torch.exp2((e - 1 - bits).float())


@pytest.mark.parametrize("M,N", SHAPES)
def test_scale_fwd(cuda, M, N):
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(M * 7 + N)
    z = torch.randn(M, N, device=cuda, generator=g).to(K.ELEM)
    resid = torch.randn(M, N, device=cuda, generator=g).to(K.ELEM)
    bias = torch.randn(N, device=cuda, generator=g).to(K.ELEM)
    gv = torch.exp2(torch.rand(N, device=cuda, generator=g) * 2 - 1)
    for rp in ([M, M // 2] if M % 2 == 0 else [M]):
        for b in (None, bias):
            for rs in (None, resid):
                (y,), check = P.guarded(M, [N], device=cuda)
                K.dora_scale_fwd(z, gv, bias=b, resid=rs, rows_policy=rp, out=y)
                torch.cuda.synchronize()
                check(f"pso_dora_scale_fwd M={M} N={N} rows_policy={rp}")
                ref = z.float().clone()
                ref[:rp] *= gv
                plain = z.float()
                if b is not None:
                    ref, plain = ref + b.float(), plain + b.float()
                if rs is not None:
                    ref, plain = ref + rs.float(), plain + rs.float()
                tag = (M, N, rp, b is not None, rs is not None)
                assert ((y.float() - ref).abs() <= _ulp(ref, K.ELEM))[:rp].all(), tag
                assert torch.equal(_bits(y[rp:]), _bits(plain[rp:].to(K.ELEM))), tag
                if b is None and rs is None:  # a single product: no contraction to allow for
                    assert torch.equal(_bits(y), _bits(ref.to(K.ELEM))), tag


def test_scale_fwd_strided_views_and_argument_checks(cuda):
    """z as a column slice of a wider matrix (the width-batched text K / V), and the entry's alignment rules."""
    from pairwise_sample_optimization_amd import _lib, kernels as K
    g = _gen(3)
    big = torch.randn(154, 4 * 128, device=cuda, generator=g).to(K.ELEM)
    gv = torch.exp2(torch.rand(128, device=cuda, generator=g) * 2 - 1)
    z = big[:, 256:384]
    y = K.dora_scale_fwd(z, gv)
    assert torch.equal(_bits(y), _bits((z.float() * gv).to(K.ELEM)))
    with pytest.raises(_lib.PsoLibError, match="16-B aligned rows"):
        K.dora_scale_fwd(big[:, 4:132], gv)
    with pytest.raises(_lib.PsoLibError, match="16-B aligned rows"):
        K.dora_scale_fwd(big[:, :132], torch.ones(132, device=cuda))
    dm = torch.zeros(128, device=cuda)
    with pytest.raises(_lib.PsoLibError, match="16-B aligned rows"):
        K.dora_bwd(big[:, 4:132], z, gv, gv, dm)


@pytest.mark.parametrize("M,N", SHAPES)
def test_bwd_kernel(cuda, M, N):
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(M * 5 + N)
    dy = torch.randn(M, N, device=cuda, generator=g).to(K.ELEM)
    z = torch.randn(M, N, device=cuda, generator=g).to(K.ELEM)
    n = torch.exp2(torch.rand(N, device=cuda, generator=g) * 2 - 1)
    gv = torch.exp2(torch.rand(N, device=cuda, generator=g) * 2 - 1)
    dm, ck_dm = _vec(N, cuda)
    dm.zero_()
    (dyg,), check = P.guarded(M, [N], device=cuda)
    dy0 = dy.clone()
    K.dora_bwd(dy, z, gv, n, dm, out=dyg)
    torch.cuda.synchronize()
    check(f"pso_dora_bwd dy_g M={M} N={N}")
    ck_dm(f"pso_dora_bwd dm M={M} N={N}")
    assert torch.equal(dy, dy0)  # out of place: dy still feeds the residual path
    assert torch.equal(_bits(dyg), _bits((gv * dy.float()).to(K.ELEM)))
    prod = dy.double() * z.double()
    dm64, bound = prod.sum(0) / n.double(), 1e-5 * prod.abs().sum(0) / n.double()
    worst = ((dm.double() - dm64).abs() / bound).max().item()
    print(f"\n  M={M} N={N}: max |dm - dm64| / bound = {worst:.3e}")
    assert worst <= 1.0
    # a second call accumulates: prev + dm, one fp32 add; and the same bits from a fresh buffer
    first = dm.clone()
    K.dora_bwd(dy, z, gv, n, dm, out=dyg)
    again = torch.zeros(N, device=cuda)
    K.dora_bwd(dy, z, gv, n, again)
    torch.cuda.synchronize()
    check("pso_dora_bwd dy_g (second call)")
    ck_dm("pso_dora_bwd dm (second call)")
    assert torch.equal(_bits(again), _bits(first))
    assert torch.equal(_bits(dm), _bits(first + first))


# ----------------------------------------------------------------------------------------------------------------------
# UNet parity against the fp32 oracle
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(which, r):
    return dora_ref.gpu_parity_case(which, r)


@pytest.mark.parametrize("which,r", [("tiny16", 8), ("sdxl32", 8), ("tiny16", 4)])
def test_unet_dora_parity(cuda, which, r):
    """eps and the gradients of every A, B and m against the oracle, at the bars tests/test_gpu_unet.py sets for the
    same shapes; first, from the oracle alone, that the case would catch a path that dropped the column scale."""
    c = _case(which, r)
    assert c.moved_eps >= 3 * dora_ref.FWD_BAR, c.moved_eps
    assert c.moved_grad >= 10 * dora_ref.GRAD_BAR, c.moved_grad
    assert set(c.mine) == set(c.ref) and len(c.mkeys) * 3 == len(c.ref)  # no tensor is left out
    assert torch.isfinite(c.out).all() and all(torch.isfinite(v).all() for v in c.mine.values())
    assert c.dora_eps < dora_ref.FWD_BAR, (c.dora_eps, c.lora_eps)
    assert c.dora_grad < dora_ref.GRAD_BAR, (c.dora_grad, c.lora_grad)
    assert c.mag_grad < dora_ref.GRAD_BAR, c.mag_grad


@pytest.mark.parametrize("which", ["tiny16", "sdxl32"])
def test_paired_pass_with_dora(cuda, which):
    """tests/test_gpu_unet.py::test_paired_pass_equals_separate_passes with DoRA adapters, same bars: the reference
    half is the adapters-off pass (no column scale reaches it), the backward is the policy-only backward."""
    from pairwise_sample_optimization_amd import kernels as K
    c = _case(which, 8)
    unet, st = c.unet, c.unet.lora
    assert st.dora
    x = K.nchw_to_nhwc(c.sample)
    B = x.shape[0]
    both, rt = unet.forward_nhwc(x, c.t, c.enc, c.text, c.tid, save=True, paired_ref=True)
    dout = torch.randn_like(both[:B].float()).to(K.ELEM)
    st.grad.zero_()
    unet.backward_nhwc(dout, rt)
    g_pair = st.grad.clone()
    pol, rt1 = unet.forward_nhwc(x, c.t, c.enc, c.text, c.tid, save=True)
    st.grad.zero_()
    unet.backward_nhwc(dout, rt1)
    g_sep = st.grad.clone()
    st.grad.zero_()
    unet.disable_adapters()
    with torch.no_grad():
        ref, _ = unet.forward_nhwc(x, c.t, c.enc, c.text, c.tid)
    unet.enable_adapters()
    rel = dora_ref._rel
    e_pol, e_ref, e_g = rel(both[:B], pol), rel(both[B:], ref), rel(g_pair, g_sep)
    mk = torch.cat([st.magnitude_view(g_pair, nm) for nm in st.adapter_names()])
    ms = torch.cat([st.magnitude_view(g_sep, nm) for nm in st.adapter_names()])
    print(f"\n  {which}: paired vs separate: policy {e_pol:.2e} reference {e_ref:.2e} grads {e_g:.2e} "
          f"(magnitudes {rel(mk, ms):.2e})")
    assert both.shape[0] == 2 * B
    assert e_pol < 1e-2 and e_ref < 1e-2 and e_g < 3e-2 and rel(mk, ms) < 3e-2
    assert (both[B:] - both[:B]).abs().max().item() > 0


def test_initial_magnitudes_start_as_plain_lora(cuda):
    """add_adapter sets m to the base weights' row norms (B = 0): g is exactly 1, and the first forward equals the
    adapters-off one up to the extra rounding of z."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel(cfg).init_weights(0).to(cuda)
    st = unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=True), allow_dora=True)
    assert torch.equal(st.dora_g, torch.ones_like(st.dora_g))
    for name, W in unet._adapted_weights().items():
        m = st.magnitude_view(st.master, name)
        assert torch.allclose(m, W.float().norm(dim=1), rtol=1e-5, atol=0), name
    g = _gen(0)
    sample = torch.randn(2, 4, 16, 16, device=cuda, generator=g)
    t = torch.tensor([999.0, 499.0], device=cuda)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, device=cuda, generator=g).bfloat16()
    add = {"text_embeds": torch.randn(2, cfg.text_embed_dim, device=cuda, generator=g).bfloat16(),
           "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2, device=cuda)}
    with torch.no_grad():
        on = unet(sample, t, enc, added_cond_kwargs=add).sample
        unet.disable_adapters()
        off = unet(sample, t, enc, added_cond_kwargs=add).sample
        unet.enable_adapters()
    assert torch.isfinite(on).all() and dora_ref._rel(on, off) < 1e-2


# ----------------------------------------------------------------------------------------------------------------------
# trainers: one optimizer step with the 8-bit AdamW, checkpoint round trip
# ----------------------------------------------------------------------------------------------------------------------
def _dora_unet(cuda, seed=1):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=True), allow_dora=True)
    unet.lora.init_gaussian(seed=seed, b_std=0.05)
    unet.prepare()
    return cfg, unet


def _check_step_and_checkpoint(tr, unet, m0, other, tmp_path):
    """After one optimizer step of `tr`: every magnitude moved, g = m / n of the new masters, and a checkpoint that
    carries the magnitudes and their moments bit for bit into `other` (a trainer of the same kind, other values)."""
    from safetensors.torch import load_file
    from pairwise_sample_optimization_amd import lora_io
    st = unet.lora
    torch.cuda.synchronize()
    assert tr.opt_step == 1 and st.grad.abs().max().item() == 0.0
    sd = {k: v.float() for k, v in unet.state_dict().items()}
    names = list(st.adapter_names())
    worst = 0.0
    for name in names:
        m = st.magnitude_view(st.master, name)
        assert torch.isfinite(m).all() and not torch.equal(m, m0[name]), name
        A, B = st.adapter_views(st.master, name)
        n64 = (sd[name + ".weight"].double() + st.scale * B.double() @ A.double()).norm(dim=1)
        g64 = m.double() / n64
        worst = max(worst, ((st.norm_views(name)[1].double() - g64).abs() / g64.abs()).max().item())
    print(f"\n  g vs m / n recomputed from the masters in fp64: {worst:.3e}")
    assert worst <= 1e-6
    lora_io.save_state(tr, str(tmp_path))
    f = load_file(os.path.join(str(tmp_path), lora_io.LORA_WEIGHT_NAME))
    assert len(f) == 3 * len(names)
    assert sum(k.endswith(".lora_magnitude_vector.weight") for k in f) == len(names)
    o = other.unet.lora
    assert not torch.equal(o.master, st.master)
    lora_io.load_state(other, str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o.master), _bits(st.master))  # A, B and m
    for name in names:
        assert torch.equal(_bits(o.magnitude_view(o.master, name)), _bits(st.magnitude_view(st.master, name)))
    assert torch.equal(_bits(o.dora_g), _bits(st.dora_g))  # load refreshes n and g
    mine, theirs = tr.adam8.tensors(), other.adam8.tensors()
    assert set(mine) == set(theirs)
    for k in mine:  # the 8-bit codes, the block absmax and the 32-bit moments of the small tensors (the magnitudes)
        assert torch.equal(mine[k].cpu(), theirs[k].cpu()), k
    assert other.opt_step == 1


def test_pso_trainer_steps_the_magnitudes(cuda, tmp_path):
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids

    def build(seed):
        cfg, unet = _dora_unet(cuda, seed)
        return cfg, unet, PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1,
                                     train_batch_size=1, lr=1e-3, use_8bit_adam=True)

    cfg, unet, tr = build(1)
    g = _gen(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).bfloat16()
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).bfloat16()
    buf = tr.sample_pairs(enc, pooled, compute_time_ids(128, 0, cuda), 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    sb = tr.shuffle(buf, generator=_gen(100))
    m0 = {nm: unet.lora.magnitude_view(unet.lora.master, nm).clone() for nm in unet.lora.adapter_names()}
    tr.train_epoch(sb)
    _check_step_and_checkpoint(tr, unet, m0, build(2)[2], tmp_path)


def test_dreambooth_trainer_steps_the_magnitudes(cuda, tmp_path):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    from pairwise_sample_optimization_amd.vae import AutoencoderKL, VAEConfig
    with torch.device(cuda):
        vae = AutoencoderKL(VAEConfig.tiny())
    vae.init_weights(2)

    def build(seed):
        cfg, unet = _dora_unet(cuda, seed)
        return cfg, unet, DreamBoothPSOTrainer(unet, vae, loss_type="pso", beta_pso=20.0, learning_rate=1e-3,
                                               gradient_accumulation_steps=1, use_8bit_adam=True)

    cfg, unet, tr = build(1)
    g = _gen(4)
    B = 2
    pix = torch.rand(2 * B, 3, 128, 128, device=cuda, generator=g) * 2 - 1
    enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).bfloat16()
    pooled = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).bfloat16()
    tid = compute_time_ids(128, 0, cuda).repeat(B, 1)
    m0 = {nm: unet.lora.magnitude_view(unet.lora.master, nm).clone() for nm in unet.lora.adapter_names()}
    loss = tr.micro_step(pix, enc, pooled, tid, generator=_gen(11))
    assert torch.isfinite(loss)
    _check_step_and_checkpoint(tr, unet, m0, build(2)[2], tmp_path)
