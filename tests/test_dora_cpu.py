"""DoRA without a GPU: the restatement tests/dora_ref.py against closed forms, the flat-bucket layout and the optimizer's
segments on a meta-device UNet, the from_args switch, and the checkpoint key converters."""
from types import SimpleNamespace

import pytest
import torch

import dora_ref


# ----------------------------------------------------------------------------------------------------------------------
# 1. the restatement against closed forms
# ----------------------------------------------------------------------------------------------------------------------
def _linear(seed=0, out=12, fin=20, r=4, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    return dict(x=rnd(7, fin), W=rnd(out, fin), A=rnd(r, fin) / r, B=0.3 * rnd(out, r), bias=rnd(out), s=0.5)


def test_zero_b_gives_the_base_weight_row_norms():
    p = _linear()
    n = dora_ref.row_norms(p["W"], p["A"], torch.zeros_like(p["B"]), p["s"])
    assert torch.equal(n, p["W"].norm(dim=1))
    n = dora_ref.row_norms(p["W"], p["A"], p["B"], p["s"])
    want = torch.stack([(p["W"][j] + p["s"] * p["B"][j] @ p["A"]).norm() for j in range(p["W"].shape[0])])
    assert torch.allclose(n, want, rtol=1e-14, atol=0)


def test_initial_magnitude_gives_plain_lora():
    p = _linear()
    n = dora_ref.row_norms(p["W"], p["A"], p["B"], p["s"])
    y = dora_ref.dora_linear(p["x"], p["W"], p["A"], p["B"], n, p["s"], p["bias"])
    lora = p["x"] @ p["W"].t() + p["s"] * (p["x"] @ p["A"].t()) @ p["B"].t() + p["bias"]
    assert torch.equal(y, lora)  # m / n == 1 exactly
    # and the fold is the same function as the written-out layer
    m = dora_ref.spread(n, torch.Generator().manual_seed(1), 1.0)
    sd2, lora2 = dora_ref.fold({"l.weight": p["W"]}, {"l.lora_A.weight": p["A"], "l.lora_B.weight": p["B"]},
                               {"l": m}, p["s"])
    yf = p["x"] @ sd2["l.weight"].t() + (p["x"] @ lora2["l.lora_A.weight"].t()) @ lora2["l.lora_B.weight"].t() \
        + p["bias"]
    yd = dora_ref.dora_linear(p["x"], p["W"], p["A"], p["B"], m, p["s"], p["bias"])
    assert torch.allclose(yf, yd, rtol=1e-13, atol=1e-13)


def test_single_linear_gradients_fp64():
    """dm against central differences; dA has no term through n: it equals the LoRA gradient on dy . g, and differs
    from the gradient of the same layer with a differentiable norm."""
    p = _linear(seed=3)
    gen = torch.Generator().manual_seed(4)
    G = torch.randn(7, 12, generator=gen, dtype=torch.float64)
    n = dora_ref.row_norms(p["W"], p["A"], p["B"], p["s"])
    m = dora_ref.spread(n, gen, 1.0).requires_grad_(True)
    A, B = p["A"].clone().requires_grad_(True), p["B"].clone().requires_grad_(True)
    loss = lambda m_, A_, B_: (dora_ref.dora_linear(p["x"], p["W"], A_, B_, m_, p["s"], p["bias"]) * G).sum()
    loss(m, A, B).backward()
    h = 1e-6
    for j in (0, 5, 11):
        e = torch.zeros_like(m)
        e[j] = h
        fd = (loss(m.detach() + e, A.detach(), B.detach()) - loss(m.detach() - e, A.detach(), B.detach())) / (2 * h)
        assert abs(fd.item() - m.grad[j].item()) <= 1e-7 * max(1.0, abs(fd.item())), (j, fd.item(), m.grad[j].item())
    z = p["x"] @ p["W"].t() + p["s"] * (p["x"] @ A.detach().t()) @ B.detach().t()
    assert torch.allclose(m.grad, (G * z).sum(0) / n, rtol=1e-12, atol=1e-12)  # the issue's dm formula
    g = (m / n).detach()
    dyg = G * g
    assert torch.allclose(A.grad, p["s"] * (dyg @ B.detach()).t() @ p["x"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(B.grad, p["s"] * dyg.t() @ (p["x"] @ A.detach().t()), rtol=1e-12, atol=1e-12)
    # a norm that is NOT detached gives another dA: the detach is a property under test, not a convenience
    A2 = p["A"].clone().requires_grad_(True)
    n_live = (p["W"] + p["s"] * (p["B"] @ A2)).norm(dim=1)
    y = (m.detach() / n_live) * (p["x"] @ p["W"].t() + p["s"] * (p["x"] @ A2.t()) @ p["B"].t()) + p["bias"]
    (y * G).sum().backward()
    assert (A2.grad - A.grad).norm() > 1e-3 * A.grad.norm()


def _tiny_oracle_setup(seed=1, r=8):
    """tiny16 UNet weights (16-bit valued, fp32) and a random peft-named LoRA dict on the CPU."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel(cfg).init_weights(0)
    st = unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    sd = {k: v.float() for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    lora = {}
    for name in st.adapter_names():
        A, B = st.adapter_views(st.master, name)
        lora[f"{name}.lora_A.weight"] = torch.randn(A.shape, generator=g) / r
        lora[f"{name}.lora_B.weight"] = torch.randn(B.shape, generator=g) * 0.05
    B_, h = 2, cfg.sample_size
    inp = dict(sample=torch.randn(B_, 4, h, h, generator=g), t=torch.tensor([999.0, 499.0]),
               enc=torch.randn(B_, 77, cfg.cross_attention_dim, generator=g),
               text=torch.randn(B_, cfg.text_embed_dim, generator=g),
               tid=torch.tensor([[128.0, 128, 0, 0, 128, 128]] * B_))
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)
    return sd, lora, inp, ocfg


def test_fold_moves_outputs_and_gradients():
    """On the tiny16 UNet through the unmodified oracle: m = n reproduces plain LoRA exactly; m = n 2^U(-1, 1) moves
    eps and the A / B gradients by far more than any parity bar, so a DoRA path that forgot its scale cannot pass."""
    from oracle import sdxl_ref
    sd, lora, inp, ocfg = _tiny_oracle_setup()
    run = lambda sd_, lora_: sdxl_ref.unet_forward(sd_, inp["sample"], inp["t"], inp["enc"], inp["text"], inp["tid"],
                                                   lora=lora_, cfg=ocfg)
    G = torch.randn(inp["sample"].shape, generator=torch.Generator().manual_seed(5))
    leaf = {k: v.clone().requires_grad_(True) for k, v in lora.items()}
    eps_lora = run(sd, leaf)
    (eps_lora * G).sum().backward()
    g_lora = {k: v.grad.clone() for k, v in leaf.items()}
    n = dora_ref.norms(sd, lora, 1.0)
    with torch.no_grad():
        eps_same = run(*dora_ref.fold(sd, lora, n, 1.0))
    assert torch.equal(eps_same, eps_lora.detach())
    gen = torch.Generator().manual_seed(6)
    mags = {p: dora_ref.spread(v, gen, 1.0).requires_grad_(True) for p, v in n.items()}
    leaf2 = {k: v.clone().requires_grad_(True) for k, v in lora.items()}
    eps_dora = run(*dora_ref.fold(sd, leaf2, mags, 1.0))
    (eps_dora * G).sum().backward()
    g_dora = {k: v.grad for k, v in leaf2.items()}
    d_eps = ((eps_dora - eps_lora).norm() / eps_lora.norm()).item()
    d_grad = dora_ref.total_rel(g_dora, g_lora)
    print(f"tiny16 oracle: DoRA vs LoRA eps {d_eps:.3e} rel, A / B gradients {d_grad:.3e} rel")
    assert d_eps > 3e-2 and d_grad > 0.25
    assert all(m.grad is not None and m.grad.abs().max() > 0 for m in mags.values())


# ----------------------------------------------------------------------------------------------------------------------
# 2. layout on the meta device
# ----------------------------------------------------------------------------------------------------------------------
def _meta_unet(sdxl=False):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        return UNet2DConditionModel(UNetConfig.sdxl() if sdxl else UNetConfig.tiny(16))


def _dora_cfg(r=8, **kw):
    return SimpleNamespace(r=r, lora_alpha=r, use_dora=True, **kw)


def test_use_dora_is_opt_in():
    from pairwise_sample_optimization_amd.unet import check_lora_config
    with pytest.raises(ValueError, match="use_dora"):
        check_lora_config(_dora_cfg())
    with pytest.raises(ValueError, match="use_dora"):
        _meta_unet().add_adapter(_dora_cfg())
    assert check_lora_config(_dora_cfg(), allow_dora=True) == (8, 8)
    with pytest.raises(ValueError, match="use_dora"):  # only the boolean True is the flag
        check_lora_config(SimpleNamespace(r=8, lora_alpha=8, use_dora="yes"), allow_dora=True)
    with pytest.raises(ValueError, match="use_rslora"):  # the other checks are unaffected
        check_lora_config(_dora_cfg(use_rslora=True), allow_dora=True)
    assert _meta_unet().add_adapter(SimpleNamespace(r=8, lora_alpha=8), allow_dora=True).dora is False


@pytest.mark.parametrize("r", [8, 4])
def test_dora_layout_adds_the_magnitudes_after_the_lora_segments(r):
    from pairwise_sample_optimization_amd.unet import LoraState
    unet = _meta_unet(sdxl=True)
    st = unet.add_adapter(_dora_cfg(r), allow_dora=True)
    plain = _meta_unet(sdxl=True).add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    assert st.dora and not plain.dora and plain.dora_g is None
    sum_c = sum(C for _, C, _ in st.blocks)
    assert st.numel == plain.numel + 8 * sum_c == st.master.numel() == st.grad.numel()
    assert st.dora_n.numel() == st.dora_g.numel() == 8 * sum_c
    assert list(st.layout) == list(plain.layout) and set(st.layout) == set(st.pad_layout)
    for path in st.layout:
        assert list(st.layout[path])[:10] == list(plain.layout[path])
        assert list(st.layout[path])[10:] == ["attn1.m_qkv", "attn1.m_o", "attn2.m_q", "attn2.m_kv", "attn2.m_o"]
        assert list(st.pad_layout[path]) == list(st.layout[path])
        C = st.layout[path]["attn1.m_o"][1]
        assert [st.layout[path][k][1:] for k in list(st.layout[path])[10:]] == [(3 * C, 1), (C, 1), (C, 1), (2 * C, 1),
                                                                                  (C, 1)]
    # a plain adapter is what LoraState(dora=False) builds: same offsets, key for key
    again = LoraState(plain.blocks, r, r, torch.device("meta"), dora=False)
    assert again.layout == plain.layout and again.pad_layout == plain.pad_layout and again.numel == plain.numel
    # ... and what it was before DoRA existed: sizes and offsets of the SDXL plain-LoRA bucket, written down
    first, second, last = ("up_blocks.1.attentions.2.transformer_blocks.1",
                           "up_blocks.1.attentions.2.transformer_blocks.0",
                           "down_blocks.1.attentions.0.transformer_blocks.0")
    assert list(plain.layout)[:2] == [first, second] and list(plain.layout)[-1] == last
    want = {8: (11612160, 11612160, {first: ((0, 24, 640), (51200, 16, 2048), (99328, 640, 8)),
                                     second: ((104448, 24, 640), (155648, 16, 2048), (203776, 640, 8)),
                                     last: ((11507712, 24, 640), (11558912, 16, 2048), (11607040, 640, 8))}),
            4: (5806080, 11612160, {first: ((0, 12, 640), (25600, 8, 2048), (49664, 640, 4)),
                                    second: ((52224, 12, 640), (77824, 8, 2048), (101888, 640, 4)),
                                    last: ((5753856, 12, 640), (5779456, 8, 2048), (5803520, 640, 4))})}[r]
    assert (plain.numel, plain.work.numel()) == want[:2]
    for path, segs in want[2].items():
        assert tuple(plain.layout[path][k] for k in ("attn1.A_qkv", "attn2.A_kv", "attn2.B_o")) == segs, path
    assert plain.pad_layout[last]["attn2.B_o"] == (11607040, 640, 8)
    assert all(len(segs) == 10 for segs in plain.layout.values())
    sd = st.state_dict_peft()
    names = list(st.adapter_names())
    assert len(sd) == 3 * len(names)
    for name in names:
        m = sd[f"{name}.lora_magnitude_vector.weight"]
        assert m.shape == (sd[f"{name}.lora_B.weight"].shape[0],)
        assert st.magnitude_view(st.grad, name).shape == m.shape
    with pytest.raises(ValueError, match="magnitude"):
        plain.magnitude_view(plain.master, names[0])
    rng = unet.grad_unit_ranges()  # asserts that consecutive units are adjacent
    assert rng[0][1] == 0 and rng[-1][1] + rng[-1][2] == st.grad.numel() and len(rng) == 11


def test_trainable_segments_list_three_tensors_per_adapter():
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.trainer import trainable_segments
    unet = _meta_unet(sdxl=True)
    st = unet.add_adapter(_dora_cfg(32), allow_dora=True)
    segs = sorted(trainable_segments(unet))
    assert len(segs) == 3 * 70 * 8
    end = 0
    for off, k in segs:
        assert off == end, "gap or overlap between parameter tensors"
        end = off + k
    assert end == st.master.numel()
    base = st.master.storage_offset()
    for name in st.adapter_names():
        m = st.magnitude_view(st.master, name)
        assert (m.storage_offset() - base, m.numel()) in segs
        assert m.numel() < K.Adam8State.MIN_8BIT_SIZE == 4096  # 32-bit optimizer state, as bitsandbytes keeps for them
    plain = _meta_unet(sdxl=True)
    plain.add_adapter(SimpleNamespace(r=32, lora_alpha=32))
    assert len(trainable_segments(plain)) == 2 * 70 * 8


def test_fp8_forward_and_dora_exclude_each_other():
    unet = _meta_unet()
    unet.add_adapter(_dora_cfg(), allow_dora=True)
    with pytest.raises(ValueError, match="use_dora"):
        unet.enable_fp8_forward()
    unet = _meta_unet().enable_fp8_forward()
    with pytest.raises(ValueError, match="use_dora"):
        unet.add_adapter(_dora_cfg(), allow_dora=True)


# ----------------------------------------------------------------------------------------------------------------------
# 3. DreamBoothPSOTrainer.from_args
# ----------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(loss_type="pso_db", beta_pso=5, neg_defactor=0.1, prior_loss_weight=0.5, distill_train_timesteps=4,
                learning_rate=2e-4, adam_beta1=0.9, adam_beta2=0.999, adam_weight_decay=1e-4, adam_epsilon=1e-8,
                max_grad_norm=1.0, gradient_accumulation_steps=4, use_8bit_adam=True, mixed_precision="bf16",
                optimizer="AdamW", train_text_encoder=False, with_prior_preservation=False, use_dora=False,
                do_edm_style_training=True, lr_scheduler="constant", lr_warmup_steps=0)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("adapter_dora", [False, True])
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("allow", [False, True])
def test_from_args_use_dora_matrix(adapter_dora, flag, allow):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    unet = _meta_unet()
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=adapter_dora), allow_dora=True)
    kw = dict(allow_dora=True) if allow else {}
    build = lambda: DreamBoothPSOTrainer.from_args(unet, None, _args(use_dora=flag), **kw)
    if (not allow and flag) or (allow and flag != adapter_dora):
        with pytest.raises(ValueError, match="use_dora"):
            build()
        return
    tr = build()
    assert tr.adam8.n == unet.lora.master.numel()
    assert len(tr.adam8.rows) >= (3 if adapter_dora else 2) * len(list(unet.lora.adapter_names()))


# ----------------------------------------------------------------------------------------------------------------------
# 4. checkpoint keys
# ----------------------------------------------------------------------------------------------------------------------
def test_key_converters_keep_magnitude_keys():
    from pairwise_sample_optimization_amd import lora_io
    p = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    sd = {f"{p}.lora_A.weight": torch.zeros(1), f"{p}.lora_B.weight": torch.zeros(1),
          f"{p}.lora_magnitude_vector.weight": torch.zeros(1)}
    d = lora_io.peft_to_diffusers(sd)
    assert set(d) == {f"{p}.lora.down.weight", f"{p}.lora.up.weight", f"{p}.lora_magnitude_vector.weight"}
    assert set(lora_io.diffusers_to_peft({"unet." + k: v for k, v in d.items()})) == set(sd)
    old = {f"unet.{p}.lora_magnitude_vector": torch.zeros(1)}  # peft before 0.11: no ".weight"
    assert set(lora_io.diffusers_to_peft(old)) == {f"{p}.lora_magnitude_vector"}


def test_load_refuses_a_file_of_the_other_adapter_kind():
    from pairwise_sample_optimization_amd import lora_io
    dora, plain = _meta_unet(), _meta_unet()
    dora.add_adapter(_dora_cfg(), allow_dora=True)
    plain.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    with pytest.raises(ValueError, match="lora_magnitude_vector"):
        lora_io.load_lora_into_unet(lora_io.peft_to_diffusers(dora.lora.state_dict_peft()), None, plain)
    with pytest.raises(ValueError, match="lora_magnitude_vector"):
        lora_io.load_lora_into_unet(lora_io.peft_to_diffusers(plain.lora.state_dict_peft()), None, dora)
