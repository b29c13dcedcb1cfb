"""Merged-weight LoRA inference on the GPU: pso_lora_merge against the fp64 restatement and bound of
tests/lora_merge_ref.py and its exact cases as bit equality; then fuse_lora / unfuse_lora / merge_and_unload on the HIP
UNet -- the fused forward against the fp32 oracle, and bit identity of everything fusing must not touch."""
import functools
from types import SimpleNamespace

import pytest
import torch

import dora_ref
import lora_merge_ref as R

pytestmark = pytest.mark.gpu

bits = R.bits


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# pso_lora_merge
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.5, 0.35])
@pytest.mark.parametrize("use_g", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_merge_meets_the_bound(cuda, shape, use_g, s):
    c = R.kernel_operands(shape, use_g, cuda)
    R.run_merge([c], s, cuda)
    R.check_bound(c, s, f"{shape} g={use_g} s={s}")


@pytest.mark.parametrize("s", [0.5, 0.35])
@pytest.mark.parametrize("use_g", [False, True])
def test_five_records_in_one_launch(cuda, use_g, s):
    cs = [R.kernel_operands(shape, use_g, cuda, seed=1) for shape in R.SHAPES]
    R.run_merge(cs, s, cuda)
    for c in cs:
        R.check_bound(c, s, f"{c.shape} g={use_g} s={s} five-record launch")
    # the same records one by one give the same bits: a record's result does not depend on its neighbours
    for c in cs:
        both = bits(c.O).clone()
        c.O.zero_()
        R.run_merge([c], s, cuda)
        assert torch.equal(bits(c.O), both), c.shape


@pytest.mark.parametrize("shape", R.SHAPES)
def test_zero_b_keeps_the_bits_of_w(cuda, shape):
    """B = 0 without g: O's bits are W's, a -0 included (the kernel leaves W alone where the adapter term is 0)."""
    c = R.kernel_operands(shape, False, cuda)
    c.B.zero_()
    c.W[0, :4] = torch.tensor([-0.0, 0.0, -1.0, 1.0], device=cuda).to(c.W.dtype)
    R.run_merge([c], 0.35, cuda)
    c.untouched()
    assert torch.equal(bits(c.O), bits(c.W))


@pytest.mark.parametrize("out,fin,r", [(5, 8, 1), (19, 260, 4), (64, 320, 8), (33, 2048, 7)])
def test_integer_case_is_exact(cuda, out, fin, r):
    """W in [-8, 8], A, B in {-1, 0, 1}, r <= 8, s = 1: every partial sum is a small integer, exact in fp32 and in
    both 16-bit types whatever the order or contraction."""
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(out + fin + r)
    W = torch.randint(-8, 9, (out, fin), device=cuda, generator=g).to(K.ELEM)
    A = torch.randint(-1, 2, (r, fin), device=cuda, generator=g).float()
    B = torch.randint(-1, 2, (out, r), device=cuda, generator=g).float()
    O = torch.empty_like(W)
    K.LoraMergeTable([(W, A, B, 1.0, None, O)], cuda).run()
    want = W.double() + B.double() @ A.double()
    assert want.abs().max().item() <= 16
    assert torch.equal(bits(O), bits(want.to(K.ELEM)))
    # ... and with a power-of-two g the product is exact too
    gv = torch.exp2(torch.randint(-2, 3, (out,), device=cuda, generator=g).float())
    K.LoraMergeTable([(W, A, B, 1.0, gv, O)], cuda).run()
    assert torch.equal(bits(O), bits((gv.double()[:, None] * want).to(K.ELEM)))


@pytest.mark.parametrize("use_g", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_scale_moves_between_s_and_b_and_runs_repeat(cuda, shape, use_g):
    """(s, B) and (s / 2, 2 B) give equal bits (both changes are exact), and so do two runs of one launch."""
    c = R.kernel_operands(shape, use_g, cuda)
    R.run_merge([c], 0.35, cuda)
    first = bits(c.O).clone()
    R.run_merge([c], 0.35, cuda)
    assert torch.equal(bits(c.O), first)
    c.B.mul_(2.0)
    R.run_merge([c], 0.175, cuda)
    c.untouched()
    assert torch.equal(bits(c.O), first)


# ----------------------------------------------------------------------------------------------------------------------
# UNet
# ----------------------------------------------------------------------------------------------------------------------
def _build(cuda, r=8, dora=False, seed=1, b_std=0.1):
    """tiny16 with an adapter of B != 0 (DoRA: magnitudes spread around n), prepared."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel(cfg).init_weights(0).to(cuda)
    st = unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r, use_dora=dora), allow_dora=True)
    if b_std is not None:
        st.init_gaussian(seed=seed, b_std=b_std)
        if dora:
            st.init_magnitudes()
            gen = _gen(7 + seed)
            for name in st.adapter_names():
                m = st.magnitude_view(st.master, name)
                m.copy_(dora_ref.spread(m.clone(), gen, 1.0))
            st.refresh()
    unet.prepare()
    return cfg, unet


def _merged(unet):
    """{adapter module path: a copy of its merged rows}."""
    return {k: v.clone() for k, v in unet._merged.dests.items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@functools.lru_cache(maxsize=None)
def _plain(r):
    return R.gpu_plain_case(r, torch.device("cuda:0"))


@pytest.mark.parametrize("r", [8, 4])
def test_fused_forward_against_the_oracle_plain_lora(cuda, r):
    """Case 1: the adapter moves the oracle's eps by at least three bars, and the fused forward meets the bar the
    adapter path has at these shapes.  On an MI355X (bf16): r = 8 the adapter moves eps by 0.139, adapter path
    8.57e-3, fused 8.46e-3; r = 4: 0.180, 8.51e-3, 8.35e-3."""
    c = _plain(r)
    assert c.moved >= 3 * R.FWD_BAR, c.moved  # from the oracle alone: a merge that dropped B A would fail below
    assert c.fused_err < R.FWD_BAR, (c.fused_err, c.adapter_err)


@functools.lru_cache(maxsize=None)
def _dora(which):
    return dora_ref.gpu_parity_case(which, 8)


@pytest.mark.parametrize("which", ["tiny16", "sdxl32"])
def test_fused_forward_against_the_oracle_dora(cuda, which):
    """Case 2: DoRA through tests/dora_ref.gpu_parity_case, whose magnitudes are spread around n.  On an MI355X (bf16): tiny16
    fused 8.83e-3 (adapter path 8.81e-3), sdxl32 9.02e-3 (9.64e-3)."""
    c = _dora(which)
    unet = c.unet
    assert unet.lora.dora and c.moved_eps >= 3 * dora_ref.FWD_BAR, c.moved_eps  # a merge without g would fail
    with pytest.raises(ValueError, match="lora_scale"):
        unet.fuse_lora(lora_scale=0.5)
    assert unet.lora_fused is False
    unet.fuse_lora()
    try:
        err = dora_ref._rel(R.eps_nograd(unet, c), c.eps32)
    finally:
        unet.unfuse_lora()
    print(f"\n  {which} DoRA: fused eps vs oracle {err:.3e} (adapter path {c.dora_eps:.3e})")
    assert err < dora_ref.FWD_BAR, (err, c.dora_eps)


@pytest.mark.parametrize("dora", [False, True])
def test_fresh_adapter_merges_to_the_base_weights(cuda, dora):
    """Case 3: B = 0 (DoRA: g == 1): the merged buffers are the base rows, the fused forward the adapter-free one."""
    cfg, unet = _build(cuda, dora=dora, b_std=None)
    c = R.tiny_inputs(cfg, cuda)
    unet.fuse_lora()
    base = unet._adapted_weights()
    assert len(unet._merged.dests) == len(base) == 8 * len(unet.lora.blocks)
    for name, W in base.items():
        assert torch.equal(bits(unet._merged.dests[name]), bits(W.data)), name
    for C, grp in unet._kv_groups.items():  # the stacked buffers as the forward reads them
        assert torch.equal(bits(unet._merged.kv[C]), bits(grp.W))
    fused = R.eps_nograd(unet, c)
    unet.disable_adapters()
    off = R.eps_nograd(unet, c)
    unet.enable_adapters()
    assert torch.equal(bits(fused), bits(off))


@pytest.mark.parametrize("dora", [False, True])
def test_training_paths_and_unfuse_keep_their_bits(cuda, dora):
    """Cases 4 and 5: save=True + backward and the paired pass give the same eps and lora.grad while fused as before;
    the fused forward differs from the adapter path; after unfuse_lora() the no-grad forward is the one before."""
    from pairwise_sample_optimization_amd import kernels as K
    cfg, unet = _build(cuda, dora=dora)
    st = unet.lora
    c = R.tiny_inputs(cfg, cuda)
    x = K.nchw_to_nhwc(c.sample)
    B = x.shape[0]
    dout = []

    def train_paths():
        res = []
        for paired in (False, True):
            st.grad.zero_()
            eps, rt = unet.forward_nhwc(x, c.t, c.enc, c.text, c.tid, save=True, paired_ref=paired)
            if not dout:
                dout.append(torch.randn(eps[:B].shape, device=cuda, generator=_gen(9)).to(K.ELEM))
            unet.backward_nhwc(dout[0], rt)
            res += [eps.clone(), st.grad.clone()]
        st.grad.zero_()
        unet.disable_adapters()
        res.append(R.eps_nograd(unet, c))
        unet.enable_adapters()
        with torch.enable_grad():  # forward() under grad mode is the autograd path, fused or not
            out = unet(c.sample, c.t, c.enc, added_cond_kwargs={"text_embeds": c.text, "time_ids": c.tid}).sample
        assert out.requires_grad
        res.append(out.detach().clone())
        return res

    before, eps_before = train_paths(), R.eps_nograd(unet, c)
    unet.fuse_lora()
    during, eps_fused = train_paths(), R.eps_nograd(unet, c)
    assert unet.lora_fused is True
    unet.unfuse_lora()
    assert unet.lora_fused is False and unet._merged is not None  # the buffers stay for the next fuse
    eps_after = R.eps_nograd(unet, c)
    for a, b in zip(before, during):
        assert torch.equal(bits(a), bits(b))
    assert before[1].abs().max().item() > 0 and before[3].abs().max().item() > 0
    assert not torch.equal(eps_fused, eps_before)  # the no-grad forward did take the merged weights
    assert torch.equal(bits(eps_after), bits(eps_before))


@pytest.mark.parametrize("dora", [False, True])
def test_refresh_and_load_peft_remerge(cuda, dora):
    """Case 6: a master update + refresh() while fused, and separately a load_peft, leave the merged buffers equal to
    those of a fresh fuse_lora() on a twin UNet, bit for bit."""
    _, a = _build(cuda, dora=dora)
    a.fuse_lora()
    first = _merged(a)
    new = _build(cuda, dora=dora, seed=2)[1].lora
    a.lora.master.copy_(new.master)
    a.lora.refresh()
    _, twin = _build(cuda, dora=dora)
    twin.lora.master.copy_(new.master)
    twin.lora.refresh()
    assert twin._merged is None  # nothing is built before the first fuse
    twin.fuse_lora()
    assert _same(_merged(a), _merged(twin)) and not _same(_merged(a), first)
    third = _build(cuda, dora=dora, seed=3)[1].lora.state_dict_peft()
    a.lora.load_peft(third)
    _, twin2 = _build(cuda, dora=dora)
    twin2.lora.load_peft(third)
    twin2.fuse_lora()
    assert _same(_merged(a), _merged(twin2)) and not _same(_merged(a), _merged(twin))
    # a second fuse_lora() at the same version and scale launches nothing: the buffers may be scribbled on
    ver = a.lora.merge_version
    some = next(iter(a._merged.dests.values()))
    some.zero_()
    a.fuse_lora()
    assert a.lora.merge_version == ver == a.lora.version and some.abs().max().item() == 0
    a.lora.refresh()
    assert _same(_merged(a), _merged(twin2))


def test_prepare_rebinds_and_a_moved_weight_raises(cuda):
    cfg, unet = _build(cuda)
    unet.fuse_lora()
    want = _merged(unet)
    lin = unet.mid_block.attentions[0].transformer_blocks[0].attn1.to_q
    lin.weight.data = lin.weight.data.clone()  # the parameter moved
    with pytest.raises(RuntimeError, match="prepare"):
        unet.lora.refresh()
    unet.prepare()
    assert unet.lora_fused and _same(_merged(unet), want)


def test_lora_scale(cuda):
    """Case 7: fuse_lora(lora_scale=0.5) = scale 1 with B halved, bit for bit."""
    _, a = _build(cuda)
    a.fuse_lora(lora_scale=0.5)
    _, b = _build(cuda)
    for name in b.lora.adapter_names():
        b.lora.adapter_views(b.lora.master, name)[1].mul_(0.5)
    b.lora.refresh()
    b.fuse_lora()
    assert _same(_merged(a), _merged(b))
    half = _merged(a)
    a.fuse_lora()  # another scale re-merges at the same adapter version
    assert not _same(_merged(a), half)


def test_errors(cuda):
    """Case 8."""
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    bare = UNet2DConditionModel(UNetConfig.tiny(16)).init_weights(0).to(cuda)
    with pytest.raises(ValueError, match="no LoRA adapter"):
        bare.fuse_lora()
    if not _lib.F16:  # full-UNet training and the fp8 forward exist on the bf16 library only
        bare.enable_full_grads()
        with pytest.raises(ValueError, match="no LoRA adapter"):
            bare.fuse_lora()
        _, unet = _build(cuda)
        unet.enable_fp8_forward(True)
        with pytest.raises(ValueError, match="enable_fp8_forward"):
            unet.fuse_lora()
        assert unet.lora_fused is False and unet._merged is None
        unet.enable_fp8_forward(False)
        unet.fuse_lora()
        with pytest.raises(ValueError, match="unfuse_lora"):
            unet.enable_fp8_forward(True)
        assert unet.fp8 is False
    _, dora = _build(cuda, dora=True)
    with pytest.raises(ValueError, match="lora_scale"):
        dora.fuse_lora(lora_scale=0.5)
    assert dora.lora_fused is False


@pytest.mark.parametrize("dora", [False, True])
def test_merge_and_unload(cuda, dora, tmp_path):
    """Case 9."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel
    cfg, unet = _build(cuda, dora=dora)
    c = R.tiny_inputs(cfg, cuda)
    unet.fuse_lora()
    eps_fused, want = R.eps_nograd(unet, c), _merged(unet)
    unet.unfuse_lora()
    assert unet.merge_and_unload() is unet
    assert unet.lora is None and unet.lora_fused is False and unet._merged is None
    for name, W in unet._adapted_weights().items():
        assert torch.equal(bits(W.data), bits(want[name])), name
    assert torch.equal(bits(R.eps_nograd(unet, c)), bits(eps_fused))
    assert not any("lora" in k for k in unet.state_dict())
    unet.save_pretrained(str(tmp_path))
    again = UNet2DConditionModel.from_pretrained(str(tmp_path)).to(cuda)
    assert again.lora is None
    assert torch.equal(bits(R.eps_nograd(again, c)), bits(eps_fused))


def test_trainer_fused_sampling(cuda):
    """Case 10: fused inside sample_pairs, unfused after it (also when the reward raises), and a micro-step on one
    fixed buffer gives the gradients of a twin trainer built without the keyword, bit for bit."""
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids

    def build(**kw):
        cfg, unet = _build(cuda, b_std=0.05)
        return cfg, unet, PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1,
                                     train_batch_size=1, **kw)

    cfg, unet, tr = build(fused_sampling=True)
    _, unet0, tr0 = build()
    assert tr.fused_sampling is True and tr0.fused_sampling is False
    g = _gen(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).to(unet.lora.work.dtype)
    tid = compute_time_ids(128, 0, cuda)
    seen = []

    def reward(x, u=unet):
        seen.append(u.lora_fused)
        return torch.rand(x.shape[0], device=cuda, generator=g)

    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g, reward_fn=reward)
    assert seen == [True] and unet.lora_fused is False and unet.lora.merge_on is False
    tr0.sample_pairs(enc, pooled, tid, 16, generator=_gen(3), reward_fn=lambda x: reward(x, unet0))
    assert seen == [True, False] and unet0._merged is None  # the default builds nothing

    def boom(x):
        raise KeyError("reward failed")

    with pytest.raises(KeyError):
        tr.sample_pairs(enc, pooled, tid, 16, generator=g, reward_fn=boom)
    assert unet.lora_fused is False
    sb = tr.shuffle(buf, generator=_gen(100))
    grads = []
    for t_, u_ in ((tr, unet), (tr0, unet0)):
        t_.auto_step = False
        u_.lora.grad.zero_()
        loss = t_.micro_step(t_.micro_batch(sb, 0))
        grads.append((loss.clone(), u_.lora.grad.clone()))
    assert torch.equal(bits(grads[0][0]), bits(grads[1][0])) and torch.equal(bits(grads[0][1]), bits(grads[1][1]))
    assert grads[0][1].abs().max().item() > 0
