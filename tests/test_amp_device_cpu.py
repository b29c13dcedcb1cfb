"""CPU checks of the device loss scaler's boundary and of the DreamBooth front door: the new C-ABI symbols are
declared, exported by all three libraries and bound with matching arity; amp.DeviceLossScaler validates its arguments
as amp.LossScaler does; DreamBoothPSOTrainer.from_args honours or rejects every flag it reads; checkpoints carry a
scaler's state as additive keys."""
import json
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pairwise_sample_optimization_amd")
NEW = ["pso_amp_unscale_clip", "pso_amp_update", "pso_adamw_step", "pso_adamw8bit_step"]


def test_new_symbols_are_declared_exported_and_bound():
    from pairwise_sample_optimization_amd import _lib
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"(pso_\w+)\(([^)]*)\);", h)}
    for lib in ("libpso_amd.so", "libpso_amd_knobs.so", "libpso_amd_f16.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, lib)]).decode()
        exported = set(re.findall(r" T (pso_\w+)", out))
        assert not set(NEW) - exported, (lib, sorted(set(NEW) - exported))
    for name in NEW:
        assert name in decl and name in _lib.SIGNATURES, name
        assert len([a for a in decl[name].split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib().pso_abi_version() == 2
    # the word indices of the state block, header against binding
    words = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PSO_AMP_(\w+) (\d+)", h)}
    assert words.pop("WORDS") == _lib.AMP_WORDS == 16
    assert words == {k[4:]: getattr(_lib, k) for k in dir(_lib)
                     if k.startswith("AMP_") and k not in ("AMP_WORDS", "AMP_INT_WORDS")}
    assert sorted(words.values()) == list(range(len(words))) and len(words) <= _lib.AMP_WORDS


@pytest.mark.parametrize("kw", [dict(init_scale=0.0), dict(init_scale=-1.0), dict(growth_factor=1.0),
                                dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(growth_interval=0)])
def test_device_scaler_argument_validation(kw):
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler, LossScaler
    with pytest.raises(ValueError):
        LossScaler(**kw)
    with pytest.raises(ValueError):  # before any device is touched
        DeviceLossScaler(**kw)


def test_device_scaler_state_block_and_make_scaler():
    """The block is plain data: built on the host, it can live on any torch device (here the CPU)."""
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler, LossScaler, make_scaler
    sc = DeviceLossScaler(device="cpu")
    assert (sc.scale, sc.growth_factor, sc.backoff_factor, sc.growth_interval) == (65536.0, 2.0, 0.5, 2000)
    assert sc.state.dtype == torch.int32 and sc.state.numel() == _lib.AMP_WORDS
    assert sc.state.view(torch.float32)[_lib.AMP_INV_SCALE].item() == 2.0 ** -16
    assert (sc.growth_tracker, sc.skipped, sc.step) == (0, 0, 0)
    assert sc.scale_word.data_ptr() == sc.state.data_ptr() + 4 * _lib.AMP_SCALE and sc.scale_word.dtype == torch.float32
    sc.scale = 1024.0
    sc.step = 5
    host = LossScaler(init_scale=8.0, growth_interval=7)
    host.growth_tracker = 3
    sd = sc.state_dict()
    assert sd["scale"] == 1024.0 and sd["step"] == 5 and set(host.state_dict()) <= set(sd)
    sc.load_state_dict(host.state_dict())  # a host scaler's checkpoint: the counts it lacks are kept
    assert (sc.scale, sc.growth_interval, sc.growth_tracker, sc.step) == (8.0, 7, 3, 5)
    assert sc.state.view(torch.float32)[_lib.AMP_INV_SCALE].item() == 0.125
    host.load_state_dict(sd)  # and the other way round
    assert host.scale == 1024.0 and host.growth_interval == 2000
    assert make_scaler(sc) is sc and make_scaler(None) is None and make_scaler(4.0).scale == 4.0


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


def test_from_args_honours_the_recipe():
    """Under the default (bf16) library: the documented substitute, no scaler, whatever mixed_precision says."""
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    unet = _unet()
    tr = DreamBoothPSOTrainer.from_args(unet, None, _args(learning_rate=3e-4, adam_beta2=0.99, max_grad_norm=0.5,
                                                          neg_defactor=0.2))
    assert (tr.loss_type, tr.beta, tr.nd, tr.prior_w, tr.distill_steps) == ("pso_db", 5.0, 0.2, 0.5, 4)
    assert (tr.lr, tr.betas, tr.wd, tr.adam_eps, tr.max_grad_norm, tr.gas) == (3e-4, (0.9, 0.99), 1e-4, 1e-8, 0.5, 4)
    assert tr.scaler is None and tr.loss_scale == 1.0 and tr.adam8 is None and tr.opt_step == 0
    assert tr.exp_avg.shape == unet.lora.master.shape
    tr = DreamBoothPSOTrainer.from_args(unet, None, _args(loss_type="pso", use_8bit_adam=True, mixed_precision="bf16"))
    assert tr.loss_type == "pso" and tr.adam8 is not None and tr.exp_avg is None
    assert tr.adam8.desc is not None and tr.adam8.n == unet.lora.master.numel()
    with pytest.raises(ValueError, match="PSO_LIB=f16"):  # a scaler belongs to the f16 library
        DreamBoothPSOTrainer.from_args(unet, None, _args(), loss_scale=1024.0)
    with pytest.raises(ValueError, match="PSO_LIB=f16"):
        DreamBoothPSOTrainer(unet, None, loss_scale=1024.0)
    with pytest.raises(ValueError, match="Unknown loss type"):  # the script's own default, DB:1929
        DreamBoothPSOTrainer.from_args(unet, None, _args(loss_type="sigmoid"))


@pytest.mark.parametrize("flag,value", [("optimizer", "prodigy"), ("train_text_encoder", True),
                                        ("with_prior_preservation", True), ("use_dora", True),
                                        ("do_edm_style_training", False), ("lr_scheduler", "cosine"),
                                        ("lr_warmup_steps", 500)])
def test_from_args_rejects_what_it_does_not_train(flag, value):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    with pytest.raises(ValueError, match=flag):
        DreamBoothPSOTrainer.from_args(_unet(), None, _args(**{flag: value}))


def _fake_trainer(scaler):
    n = 64
    lora = SimpleNamespace(r=8, state_dict_peft=lambda: {"a.attn1.to_q.lora_A.weight": torch.ones(8, 4),
                                                         "a.attn1.to_q.lora_B.weight": torch.zeros(4, 8)})
    return SimpleNamespace(unet=SimpleNamespace(lora=lora), exp_avg=torch.rand(n), exp_avg_sq=torch.rand(n),
                           opt_step=3, n_micro=12, scaler=scaler)


def test_checkpoint_carries_the_scaler_state(tmp_path, monkeypatch):
    from pairwise_sample_optimization_amd import lora_io
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler, LossScaler
    monkeypatch.setattr(lora_io, "load_lora_into_unet", lambda *a, **k: None)  # the LoRA file is not tested here
    src = LossScaler(init_scale=512.0, growth_interval=5)
    src.update(False)
    src.update(False)
    t1 = _fake_trainer(src)
    lora_io.save_state(t1, str(tmp_path))
    meta = json.load(open(tmp_path / "pso_state.json"))
    assert meta["loss_scaler"] == src.state_dict() and meta["opt_step"] == 3  # additive: the old keys are all there
    t2 = _fake_trainer(LossScaler())
    t2.opt_step = t2.n_micro = 0
    lora_io.load_state(t2, str(tmp_path))
    assert t2.scaler.state_dict() == src.state_dict() and (t2.opt_step, t2.n_micro) == (3, 12)
    assert torch.equal(t2.exp_avg, t1.exp_avg)
    t3 = _fake_trainer(DeviceLossScaler(device="cpu"))  # a host scaler's checkpoint into a device scaler
    lora_io.load_state(t3, str(tmp_path))
    assert (t3.scaler.scale, t3.scaler.growth_interval, t3.scaler.growth_tracker) == (512.0, 5, 2)
    t4 = _fake_trainer(None)  # a trainer without a scaler ignores the key
    lora_io.load_state(t4, str(tmp_path))
    assert t4.opt_step == 3
    # an old-format checkpoint (no loss_scaler key) still loads and leaves the scaler as constructed
    del meta["loss_scaler"]
    json.dump(meta, open(tmp_path / "pso_state.json", "w"))
    t5 = _fake_trainer(LossScaler(init_scale=64.0))
    t5.opt_step = 0
    lora_io.load_state(t5, str(tmp_path))
    assert t5.scaler.scale == 64.0 and t5.scaler.growth_tracker == 0 and t5.opt_step == 3
