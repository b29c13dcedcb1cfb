"""CPU checks of the Prodigy optimizer: the numpy restatement (tests/prodigy_ref.py) against closed forms, and the host
plumbing -- the trainers' arguments, DreamBoothPSOTrainer.from_args, PSOTrainer.from_config and the checkpoint format.
The kernels (csrc/prodigy.hip) are checked against the restatement in tests/test_gpu_prodigy.py; that the new entry
points are exported and bound is tests/test_abi.py's check of every declaration in include/pso_amd.h."""
import json
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from prodigy_ref import ProdigyRef


def test_closed_form_first_two_steps():
    """Constant gradient with |g_i| >= 1, lr 1, eps 0, no weight decay, no bias correction, no safeguard.
    Step 1: p = p0, so the numerator is 0, d_hat = 0 and d stays d0 exactly; every parameter moves by
    d0 (1 - b1) / sqrt(1 - b2) against its gradient's sign.  Step 2: num = d0 sum|g| * that distance and
    den = d0 (1 + b3) sum|g|, so d = d0 (1 - b1) / sqrt(1 - b2) / (1 + b3): about 1.5815 d0 at the defaults."""
    rng = np.random.default_rng(0)
    g = (rng.uniform(1.0, 3.0, 257) * rng.choice([-1.0, 1.0], 257)).astype(np.float32)
    # parameters start at 0: the first move of 3e-6 is then kept to float32 precision, not to an ulp of a unit-scale p
    r = ProdigyRef(np.zeros(257), lr=1.0, eps=0.0, weight_decay=0.0)
    d0 = r.d0
    assert d0 == 1e-6
    r.step(g)
    assert r.d == d0 and r.d_max == d0 and r.k == 1 and r.updated == 1 and r.d_numerator == 0.0
    b1, b2, b3 = float(r.b1), float(r.b2), float(r.b3)
    move = d0 * (1.0 - b1) / math.sqrt(1.0 - b2)
    np.testing.assert_allclose(r.p0 - r.p, move * np.sign(g), rtol=1e-6)
    r.step(g)
    want = d0 * (1.0 - b1) / math.sqrt(1.0 - b2) / (1.0 + b3)
    assert abs(r.d - want) <= 1e-6 * want, (r.d, want)
    assert abs(r.d / d0 - 1.5815) < 1e-3 and r.k == 2 and r.d_max == r.d


def test_zero_gradient_changes_nothing_but_the_moments():
    rng = np.random.default_rng(1)
    r = ProdigyRef(rng.standard_normal(64), lr=1.0, weight_decay=1e-2, d0=1e-3)
    g = rng.standard_normal(64).astype(np.float32)
    r.step(g)
    r.step(g)
    p, m, d, k, dnum = r.p.copy(), r.m.copy(), r.d, r.k, r.d_numerator
    r.s[:] = 0  # a run that starts from rest: s is what the denominator sums
    r.step(np.zeros(64, np.float32))
    assert r.p.tobytes() == p.tobytes() and (r.d, r.k, r.d_numerator) == (d, k, dnum) and r.updated == 0
    assert r.m.tobytes() == (r.b1 * m).tobytes()
    fresh = ProdigyRef(rng.standard_normal(8))
    fresh.step(np.zeros(8, np.float32))
    assert fresh.k == 0 and fresh.d == fresh.d0 and fresh.p.tobytes() == fresh.p0.tobytes()


def test_beta3_defaults_to_sqrt_beta2_and_weight_decay_forms_differ():
    rng = np.random.default_rng(2)
    p, g = rng.standard_normal(32), rng.standard_normal(32).astype(np.float32)
    assert ProdigyRef(p, betas=(0.9, 0.99)).b3 == np.float32(math.sqrt(0.99))
    assert ProdigyRef(p, betas=(0.9, 0.99), beta3=0.5).b3 == np.float32(0.5)
    runs = []
    for decouple in (True, False):
        r = ProdigyRef(p, lr=1.0, weight_decay=0.1, decouple=decouple, d0=1e-2)
        for _ in range(4):
            r.step(g)
        runs.append(r.p)
    assert np.abs(runs[0] - runs[1]).max() > 0


# ---- host plumbing ---------------------------------------------------------------------------------------------------
def _unet():
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    return unet


def _args(**kw):
    """The recipe personalization/scripts/pso_dog.sh as the reference's argparse namespace."""
    base = dict(loss_type="pso_db", beta_pso=5, neg_defactor=0.1, prior_loss_weight=0.5, distill_train_timesteps=4,
                learning_rate=2e-4, adam_beta1=0.9, adam_beta2=0.999, adam_weight_decay=1e-4, adam_epsilon=1e-8,
                max_grad_norm=1.0, gradient_accumulation_steps=4, use_8bit_adam=False, mixed_precision="fp16",
                optimizer="AdamW", train_text_encoder=False, with_prior_preservation=False, use_dora=False,
                do_edm_style_training=True, lr_scheduler="constant", lr_warmup_steps=0)
    base.update(kw)
    return SimpleNamespace(**base)


def _from_args(**kw):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    unet = _unet()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = DreamBoothPSOTrainer.from_args(unet, None, _args(**kw), allow_prodigy=True)
    return unet, tr, [str(x.message) for x in w]


def test_from_args_trains_prodigy_on_request_only():
    """Without allow_prodigy=True the refusal of --optimizer prodigy stands as before
    (tests/test_amp_device_cpu.py::test_from_args_rejects_what_it_does_not_train pins it); the gate is about Prodigy
    alone."""
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    with pytest.raises(ValueError, match="allow_prodigy=True"):
        DreamBoothPSOTrainer.from_args(_unet(), None, _args(optimizer="prodigy", learning_rate=1.0))
    tr = DreamBoothPSOTrainer.from_args(_unet(), None, _args(optimizer="prodigy", learning_rate=1.0),
                                        allow_prodigy=True)
    assert tr.optimizer == "prodigy"
    assert DreamBoothPSOTrainer.from_args(_unet(), None, _args()).optimizer == "adamw"


def test_from_args_accepts_prodigy_and_maps_the_flags():
    unet, tr, msgs = _from_args(optimizer="prodigy", learning_rate=1.0, adam_beta1=0.8, adam_beta2=0.99,
                                adam_weight_decay=1e-3, adam_epsilon=1e-7)
    assert msgs == []
    assert tr.optimizer == "prodigy" and tr.adam8 is None and tr.opt_step == 0
    assert (tr.lr, tr.betas, tr.wd, tr.adam_eps) == (1.0, (0.8, 0.99), 1e-3, 1e-7)
    # the script's defaults (DB:641-673): beta3 None, the three switches on; d0 / d_coef / growth_rate prodigyopt's
    assert tr.prodigy_opts == dict(beta3=None, decouple=True, use_bias_correction=True, safeguard_warmup=True,
                                   d_coef=1.0, growth_rate=float("inf"))
    n = unet.lora.master.numel()
    ts = tr.prodigy.tensors()
    assert set(ts) == {"p0", "exp_avg", "exp_avg_sq", "s", "prodigy_state"}
    assert all(ts[k].numel() == n and ts[k].dtype == torch.float32 for k in ("p0", "exp_avg", "exp_avg_sq", "s"))
    assert tr.exp_avg is tr.prodigy.exp_avg and tr.exp_avg_sq is tr.prodigy.exp_avg_sq
    _, tr, _ = _from_args(optimizer="Prodigy", learning_rate=1.0, prodigy_beta3=0.9, prodigy_decouple=False,
                          prodigy_use_bias_correction=False, prodigy_safeguard_warmup=False)
    assert tr.optimizer == "prodigy"
    assert tr.prodigy_opts == dict(beta3=0.9, decouple=False, use_bias_correction=False, safeguard_warmup=False,
                                   d_coef=1.0, growth_rate=float("inf"))


def test_from_args_prodigy_warnings_and_unknown_optimizer_fallback():
    _, tr, msgs = _from_args(optimizer="prodigy", learning_rate=1e-4)
    assert tr.optimizer == "prodigy" and len(msgs) == 1 and "around 1.0" in msgs[0]
    _, tr, msgs = _from_args(optimizer="prodigy", learning_rate=0.1)  # the bound itself warns
    assert any("around 1.0" in m for m in msgs)
    _, tr, msgs = _from_args(optimizer="prodigy", learning_rate=1.0, use_8bit_adam=True)
    assert tr.optimizer == "prodigy" and tr.adam8 is None and tr.prodigy is not None
    assert len(msgs) == 1 and "use_8bit_adam is ignored" in msgs[0]
    _, tr, msgs = _from_args(optimizer="lion")
    assert tr.optimizer == "adamw" and tr.prodigy is None and tr.exp_avg is not None
    assert len(msgs) == 1 and "Unsupported choice of optimizer" in msgs[0] and "lion" in msgs[0]
    _, tr, msgs = _from_args(optimizer="lion", use_8bit_adam=True)  # the fallback is AdamW whole: 8-bit is honoured
    assert tr.optimizer == "adamw" and tr.adam8 is not None
    _, tr, msgs = _from_args()  # AdamW as before, silently
    assert tr.optimizer == "adamw" and tr.prodigy is None and msgs == []


def test_prodigy_state_block_layout():
    """The host-side fill documented in include/pso_amd.h: d = d0 = d_max, everything else zero; the word offsets of
    _lib match the header's defines."""
    import os
    import re
    from pairwise_sample_optimization_amd import _lib, kernels as K
    st = K.ProdigyState(torch.arange(5, dtype=torch.float32), d0=1e-3)
    sc = st.scalars()
    assert sc == dict(d=1e-3, d0=1e-3, d_max=1e-3, d_numerator=0.0, d_denom=0.0, d_hat=0.0, dlr=0.0, k=0, updated=0,
                      skipped=0)
    assert st.state.dtype == torch.int32 and st.state.numel() == _lib.PRODIGY_WORDS
    assert torch.equal(st.p0, torch.arange(5, dtype=torch.float32)) and st.s.abs().max() == 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = dict(re.findall(r"#define PSO_PRODIGY_(\w+) (\d+)", open(os.path.join(root, "include", "pso_amd.h")).read()))
    assert int(hdr["WORDS"]) == _lib.PRODIGY_WORDS
    for name, w in {**_lib.PRODIGY_F64, **_lib.PRODIGY_I32}.items():
        assert int(hdr[name.upper()]) == w, name
    assert all(w % 2 == 0 for w in _lib.PRODIGY_F64.values())  # the f64 fields are 8-byte aligned in the block
    assert (int(hdr["DECOUPLE"]), int(hdr["BIAS_CORRECTION"]), int(hdr["SAFEGUARD_WARMUP"])) == (
        _lib.PRODIGY_DECOUPLE, _lib.PRODIGY_BIAS_CORRECTION, _lib.PRODIGY_SAFEGUARD_WARMUP)
    with pytest.raises(ValueError):
        K.ProdigyState(torch.zeros(4), d0=0.0)


def test_trainer_arguments_and_from_config():
    from pairwise_sample_optimization_amd.config import config_sdxl_turbo_dpo
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _unet()
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, optimizer="Prodigy", lr=1.0, prodigy_d0=1e-4,
                    prodigy_d_coef=2.0, prodigy_growth_rate=1.5, prodigy_use_bias_correction=True)
    assert tr.optimizer == "prodigy" and tr.adam8 is None and tr.opt_step == 0
    assert tr.prodigy_opts == dict(beta3=None, decouple=True, use_bias_correction=True, safeguard_warmup=False,
                                   d_coef=2.0, growth_rate=1.5)
    assert PSOTrainer(unet, mode="turbo", num_steps=2).optimizer == "adamw"
    with pytest.raises(ValueError, match="optimizer"):
        PSOTrainer(unet, mode="turbo", num_steps=2, optimizer="lion")
    seen = {}

    class Probe(PSOTrainer):
        def __init__(self, unet, **kw):  # capture what from_config resolves, build nothing
            seen.clear()
            seen.update(kw)

    c = config_sdxl_turbo_dpo.get_config()
    Probe.from_config(None, c)
    assert seen["optimizer"] == "adamw" and not any(k.startswith("prodigy_") for k in seen)  # absent keys: AdamW
    c.train["optimizer"] = "prodigy"
    c.train["prodigy_safeguard_warmup"] = True
    c.train["prodigy_beta3"] = 0.95
    Probe.from_config(None, c)
    assert seen["optimizer"] == "prodigy" and seen["prodigy_safeguard_warmup"] is True and seen["prodigy_beta3"] == 0.95
    assert "prodigy_decouple" not in seen  # left to the constructor's default


def _fake_trainer(prodigy):
    from pairwise_sample_optimization_amd import kernels as K
    lora = SimpleNamespace(r=8, state_dict_peft=lambda: {"a.attn1.to_q.lora_A.weight": torch.ones(8, 4),
                                                         "a.attn1.to_q.lora_B.weight": torch.zeros(4, 8)})
    tr = SimpleNamespace(unet=SimpleNamespace(lora=lora), opt_step=3, n_micro=12, scaler=None)
    if prodigy:
        tr.prodigy = K.ProdigyState(torch.rand(64), d0=1e-3)
        for t in (tr.prodigy.exp_avg, tr.prodigy.exp_avg_sq, tr.prodigy.s):
            t.uniform_()
        tr.prodigy.state[14] = 3  # k
        tr.exp_avg, tr.exp_avg_sq = tr.prodigy.exp_avg, tr.prodigy.exp_avg_sq
    else:
        tr.exp_avg, tr.exp_avg_sq = torch.rand(64), torch.rand(64)
    return tr


def test_checkpoint_holds_the_prodigy_state_and_names_the_optimizer(tmp_path, monkeypatch):
    from safetensors.torch import load_file
    from pairwise_sample_optimization_amd import lora_io
    monkeypatch.setattr(lora_io, "load_lora_into_unet", lambda *a, **k: None)  # the LoRA file is not tested here
    pdir, adir = tmp_path / "prodigy", tmp_path / "adamw"
    t1 = _fake_trainer(True)
    lora_io.save_state(t1, str(pdir))
    assert set(load_file(str(pdir / lora_io.OPT_NAME))) == {"p0", "exp_avg", "exp_avg_sq", "s", "prodigy_state"}
    assert json.load(open(pdir / "pso_state.json"))["optimizer"] == "prodigy"
    t2 = _fake_trainer(True)
    lora_io.load_state(t2, str(pdir))
    for k, t in t1.prodigy.tensors().items():
        assert t2.prodigy.tensors()[k].numpy().tobytes() == t.numpy().tobytes(), k
    assert t2.prodigy.scalars()["k"] == 3 and (t2.opt_step, t2.n_micro) == (3, 12)
    a1 = _fake_trainer(False)
    lora_io.save_state(a1, str(adir))
    assert json.load(open(adir / "pso_state.json"))["optimizer"] == "adamw"
    with pytest.raises(KeyError, match="Prodigy"):
        lora_io.load_state(_fake_trainer(False), str(pdir))  # a Prodigy checkpoint into an AdamW trainer
    with pytest.raises(KeyError, match="Prodigy"):
        lora_io.load_state(_fake_trainer(True), str(adir))   # and the other way round
