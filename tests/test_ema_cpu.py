"""CPU checks of the EMA of the trained weights (pairwise_sample_optimization_amd/ema.py): get_decay against
hand-derived values and against tests/ema_ref.py, the argument refusals, the state dict, the trainers' front doors, the
checkpoint rules, and the C-ABI boundary of the two new entries in all three libraries."""
import json
import math
import os
import re
import subprocess
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pairwise_sample_optimization_amd")
NEW = ["pso_ema_step", "pso_ema_swap"]


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """Building a CPU UNet draws its initial weights from torch's global generator: leave that stream as it was, so
    later test files that read it unseeded see the numbers they saw before this file existed."""
    with torch.random.fork_rng(devices=[]):
        yield


def _flat_unet(n=64, seed=0):
    """The least trainable() reads: a flat CPU master, its gradient and a refresh that counts its calls."""
    lora = SimpleNamespace(master=torch.randn(n, generator=torch.Generator().manual_seed(seed)), grad=torch.zeros(n),
                           refreshed=0)
    lora.refresh = lambda cast=True: setattr(lora, "refreshed", lora.refreshed + 1)
    return SimpleNamespace(full=None, lora=lora)


def _ema(**kw):
    from pairwise_sample_optimization_amd.ema import EMAModel
    return EMAModel(_flat_unet(), **kw)


# ----------------------------------------------------------------------------------------------------------------------
# get_decay
# ----------------------------------------------------------------------------------------------------------------------
def test_get_decay_default_form():
    e = _ema()
    assert [e.get_decay(k) for k in (1, 2, 3, 11)] == [0.0, 2 / 11, 3 / 12, 11 / 20]
    assert e.get_decay(0) == 0.0
    assert all(isinstance(e.get_decay(k), float) for k in range(5))


def test_get_decay_cap_and_floor():
    e = _ema(decay=0.5)
    assert e.get_decay(9) == 9 / 18 == 0.5 and e.get_decay(8) == 8 / 17  # (1 + 7) / (10 + 7) < 0.5: not capped yet
    assert e.get_decay(10) == 0.5 and e.get_decay(10 ** 6) == 0.5        # 10 / 19 > 0.5: capped
    assert _ema().get_decay(10 ** 9) == 0.9999
    f = _ema(min_decay=0.3)
    assert f.get_decay(2) == 0.3 and f.get_decay(3) == 0.3               # 2 / 11, 3 / 12 < 0.3: the floor
    assert f.get_decay(5) == 5 / 14                                      # 0.357: above it
    assert f.get_decay(1) == 0.0                                         # step <= 0 returns before the floor
    g = _ema(decay=0.2, min_decay=0.4)                                   # min(., decay) first, max(., min_decay) after
    assert g.get_decay(50) == 0.4


def test_get_decay_update_after_step():
    e = _ema(update_after_step=5)
    assert [e.get_decay(k) for k in range(0, 7)] == [0.0] * 7
    assert e.get_decay(7) == 2 / 11 and e.get_decay(8) == 3 / 12


def test_get_decay_warmup_form():
    e = _ema(use_ema_warmup=True, inv_gamma=1.0, power=2 / 3)
    assert e.get_decay(1) == 0.0
    assert e.get_decay(2) == 1 - (1 + 1 / 1.0) ** -(2 / 3)
    assert e.get_decay(101) == 1 - (1 + 100 / 1.0) ** -(2 / 3)
    assert abs(e.get_decay(2) - (1 - 2 ** (-2 / 3))) < 1e-15 and abs(e.get_decay(2) - 0.37003947505256341) < 1e-15
    h = _ema(use_ema_warmup=True, inv_gamma=4.0, power=0.75)
    assert h.get_decay(9) == 1 - (1 + 8 / 4.0) ** -0.75
    assert _ema(use_ema_warmup=True, power=0.0).get_decay(50) == 0.0  # (..) ** -0 = 1


def test_get_decay_matches_the_restatement():
    for kw in (dict(), dict(decay=0.9), dict(min_decay=0.25), dict(update_after_step=3),
               dict(use_ema_warmup=True), dict(use_ema_warmup=True, inv_gamma=2.5, power=0.8, decay=0.99)):
        e = _ema(**kw)
        for k in range(0, 40):
            assert e.get_decay(k) == ema_ref.get_decay(k, **kw), (kw, k)


def test_restatement_rounds_three_times():
    """s - omd (s - p) with every operation rounded to float32: differs from the double-precision expression rounded
    once on some elements, and omd = 1 does not always give p."""
    rng = np.random.default_rng(0)
    s = rng.standard_normal(4096).astype(np.float32)
    p = rng.standard_normal(4096).astype(np.float32)
    omd = ema_ref.one_minus_decay32(2 / 11)
    assert omd.dtype == np.float32 and omd == np.float32(9 / 11)
    got = ema_ref.ema_update(s, p, omd)
    once = (s.astype(np.float64) - np.float64(omd) * (s.astype(np.float64) - p.astype(np.float64))).astype(np.float32)
    assert got.dtype == np.float32 and np.abs(got - once).max() <= 1e-5 and (got != once).any()
    assert (ema_ref.ema_update(s, p, np.float32(1.0)) != p).any()
    assert np.array_equal(ema_ref.ema_update(s, p, np.float32(0.0)).view(np.int32), s.view(np.int32))


# ----------------------------------------------------------------------------------------------------------------------
# arguments and state
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, name", [(dict(decay=1.5), "decay"), (dict(decay=-0.1), "decay"),
                                      (dict(min_decay=1.01), "min_decay"), (dict(min_decay=-1e-3), "min_decay"),
                                      (dict(update_after_step=-1), "update_after_step"),
                                      (dict(inv_gamma=0.0), "inv_gamma"), (dict(inv_gamma=-2.0), "inv_gamma"),
                                      (dict(power=-0.5), "power"), (dict(decay=math.nan), "decay")])
def test_constructor_refusals_name_the_argument(kw, name):
    with pytest.raises(ValueError, match=r"EMAModel: " + name + " "):
        _ema(**kw)


def test_constructor_state():
    from pairwise_sample_optimization_amd.ema import EMAModel
    unet = _flat_unet()
    e = EMAModel(unet)
    assert (e.decay, e.min_decay, e.update_after_step, e.use_ema_warmup, e.inv_gamma, e.power) == \
        (0.9999, 0.0, 0, False, 1.0, 2 / 3)
    assert e.optimization_step == 0 and e.cur_decay_value is None and not e.swapped
    assert torch.equal(e.shadow, unet.lora.master) and e.shadow.data_ptr() != unet.lora.master.data_ptr()
    assert e.shadow.dtype == torch.float32


def test_state_dict_round_trip():
    from pairwise_sample_optimization_amd.ema import EMAModel
    a = EMAModel(_flat_unet(seed=1), decay=0.9, min_decay=0.1, update_after_step=2, use_ema_warmup=True, inv_gamma=3.0,
                 power=0.5)
    a.optimization_step = 7
    sd = a.state_dict()
    assert set(sd) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma",
                       "power", "shadow_params"}
    assert len(sd["shadow_params"]) == 1 and sd["shadow_params"][0].data_ptr() != a.shadow.data_ptr()
    b = EMAModel(_flat_unet(seed=2))
    assert not torch.equal(a.shadow, b.shadow)
    b.load_state_dict(sd)
    assert torch.equal(b.shadow.view(torch.int32), a.shadow.view(torch.int32))
    assert b.scalars() == a.scalars() == json.loads(json.dumps(a.scalars()))
    assert b.optimization_step == 7 and b.cur_decay_value == a.get_decay(7)
    assert [b.get_decay(k) for k in range(12)] == [a.get_decay(k) for k in range(12)]
    with pytest.raises(ValueError, match="shadow_params"):
        b.load_state_dict(dict(sd, shadow_params=[torch.zeros(3)]))
    with pytest.raises(ValueError, match="EMAModel: decay"):
        b.load_state_dict(dict(sd, decay=2.0))


def test_swapped_in_state_guards_without_a_launch():
    """The guards are host-side: with the flag set (no kernel runs here) step, a second swap-in, the state dict and
    both trainers' micro_step / optimizer_step raise."""
    from pairwise_sample_optimization_amd.trainer import check_ema_live, lora_optimizer_step
    e = _ema()
    with pytest.raises(RuntimeError, match="restore"):
        e.restore()  # nothing swapped in
    e.store()
    e.swapped = True
    for fn in (e.step, e.store, e.copy_to, e.state_dict):
        with pytest.raises(RuntimeError, match="swapped in"):
            fn()
    with pytest.raises(RuntimeError, match="swapped in"):
        with e.average_parameters():
            pass
    tr = SimpleNamespace(ema=e, unet=e.unet)
    with pytest.raises(RuntimeError, match="optimizer_step while the EMA weights"):
        lora_optimizer_step(tr)
    with pytest.raises(RuntimeError, match="micro_step while the EMA weights"):
        check_ema_live(tr, "micro_step")
    assert e.optimization_step == 0
    e.swapped = False
    check_ema_live(tr, "micro_step")
    check_ema_live(SimpleNamespace(), "micro_step")  # a trainer object without the attribute counts as off


# ----------------------------------------------------------------------------------------------------------------------
# the trainers' front doors
# ----------------------------------------------------------------------------------------------------------------------
def _meta_unet():
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    return unet


def _args(**kw):
    base = dict(loss_type="pso_db", beta_pso=5, neg_defactor=0.1, prior_loss_weight=0.5, distill_train_timesteps=4,
                learning_rate=2e-4, gradient_accumulation_steps=4, mixed_precision="fp16", optimizer="AdamW",
                do_edm_style_training=True, lr_scheduler="constant", lr_warmup_steps=0)
    base.update(kw)
    return SimpleNamespace(**base)


EMA_ON = dict(use_ema=True, ema_decay=0.9, ema_min_decay=0.05, ema_update_after_step=3, ema_use_warmup=True,
              ema_inv_gamma=2.0, ema_power=0.75)
WANT = {"decay": 0.9, "min_decay": 0.05, "optimization_step": 0, "update_after_step": 3, "use_ema_warmup": True,
        "inv_gamma": 2.0, "power": 0.75}


def test_trainers_default_to_no_ema():
    from pairwise_sample_optimization_amd.config import config_sdxl_dmd_dpo, config_sdxl_turbo_dpo
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _meta_unet()
    assert PSOTrainer(unet).ema is None and PSOTrainer(unet, use_ema=False, ema_decay=0.5).ema is None
    assert DreamBoothPSOTrainer(unet, None).ema is None
    assert PSOTrainer.from_config(unet, config_sdxl_turbo_dpo.get_config()).ema is None
    assert PSOTrainer.from_config(unet, config_sdxl_dmd_dpo.get_config(), mode="dmd").ema is None
    assert DreamBoothPSOTrainer.from_args(unet, None, _args()).ema is None
    assert DreamBoothPSOTrainer.from_args(unet, None, _args(use_ema=False, ema_decay=0.5)).ema is None
    for cfg in (config_sdxl_turbo_dpo.get_config(), config_sdxl_dmd_dpo.get_config()):
        assert not [k for k in cfg.train.keys() if "ema" in k]  # the reference configs carry none


def test_trainers_take_the_ema_arguments():
    from pairwise_sample_optimization_amd.config import config_sdxl_turbo_dpo
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.ema import EMAModel
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _meta_unet()
    n = unet.lora.master.numel()
    cfg = config_sdxl_turbo_dpo.get_config()
    for k, v in EMA_ON.items():
        cfg.train[k] = v
    trainers = [PSOTrainer(unet, **EMA_ON), DreamBoothPSOTrainer(unet, None, **EMA_ON),
                PSOTrainer.from_config(unet, cfg), DreamBoothPSOTrainer.from_args(unet, None, _args(**EMA_ON))]
    for tr in trainers:
        assert isinstance(tr.ema, EMAModel) and tr.ema.scalars() == WANT and tr.ema.cur_decay_value is None
        assert tr.ema.shadow.shape == (n,) and tr.ema.shadow.dtype == torch.float32 and tr.ema.unet is unet
    d = PSOTrainer(unet, use_ema=True).ema  # the defaults are diffusers'
    assert d.scalars() == {"decay": 0.9999, "min_decay": 0.0, "optimization_step": 0, "update_after_step": 0,
                           "use_ema_warmup": False, "inv_gamma": 1.0, "power": 2 / 3}
    cfg2 = config_sdxl_turbo_dpo.get_config()
    cfg2.train["use_ema"] = True  # the switch alone
    assert PSOTrainer.from_config(unet, cfg2).ema.decay == 0.9999
    assert DreamBoothPSOTrainer.from_args(unet, None, _args(use_ema=True)).ema.power == 2 / 3
    with pytest.raises(ValueError, match="EMAModel: decay"):
        PSOTrainer(unet, use_ema=True, ema_decay=1.5)
    with pytest.raises(ValueError, match="EMAModel: inv_gamma"):
        DreamBoothPSOTrainer.from_args(unet, None, _args(use_ema=True, ema_inv_gamma=0.0))


# ----------------------------------------------------------------------------------------------------------------------
# checkpoints (host code only: the LoRA load of the live adapter launches kernels and is stubbed)
# ----------------------------------------------------------------------------------------------------------------------
def _cpu_unet(dora=False):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=dora), allow_dora=True)
    return unet


def _trainer(unet, seed, with_ema=True, **kw):
    from pairwise_sample_optimization_amd.ema import EMAModel
    n = unet.lora.master.numel()
    g = torch.Generator().manual_seed(seed)
    unet.lora.master.copy_(torch.randn(n, generator=g))
    ema = None
    if with_ema:
        ema = EMAModel(unet, **kw)
        ema.shadow.copy_(torch.randn(n, generator=g))
    return SimpleNamespace(unet=unet, exp_avg=torch.rand(n, generator=g), exp_avg_sq=torch.rand(n, generator=g),
                           opt_step=3, n_micro=12, scaler=None, lr_schedule=None, lr_word=None, ema=ema)


@pytest.mark.parametrize("dora", [False, True])
def test_checkpoint_carries_the_ema(tmp_path, monkeypatch, dora):
    from safetensors.torch import load_file
    from pairwise_sample_optimization_amd import lora_io
    from pairwise_sample_optimization_amd.trainer import trainable_segments
    monkeypatch.setattr(lora_io, "load_lora_into_unet", lambda *a, **k: None)
    unet = _cpu_unet(dora)
    t1 = _trainer(unet, 1, decay=0.9, update_after_step=1)
    t1.ema.optimization_step = 5
    lora_io.save_state(t1, str(tmp_path))
    assert lora_io.EMA_LORA_WEIGHT_NAME == "pytorch_lora_weights_ema.safetensors"
    live = load_file(str(tmp_path / lora_io.LORA_WEIGHT_NAME))
    avg = load_file(str(tmp_path / lora_io.EMA_LORA_WEIGHT_NAME))
    assert set(avg) == set(live) and all(k.startswith("unet.") for k in avg)  # the same diffusers key layout
    assert any(".lora.down.weight" in k for k in avg) and any(".lora.up.weight" in k for k in avg)
    assert any("lora_magnitude_vector" in k for k in avg) == dora
    assert sum(v.numel() for v in avg.values()) == sum(n for _, n in trainable_segments(unet))
    assert any(not torch.equal(avg[k], live[k]) for k in avg)  # the shadow, not the master
    meta = json.load(open(tmp_path / "pso_state.json"))
    assert meta["ema"] == t1.ema.scalars() and meta["ema"]["optimization_step"] == 5 and "shadow_params" not in meta["ema"]
    # into a fresh trainer with an EMA of other settings: shadow and scalars are the checkpoint's, bit for bit
    t2 = _trainer(_cpu_unet(dora), 2)
    assert not torch.equal(t2.ema.shadow, t1.ema.shadow)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lora_io.load_state(t2, str(tmp_path))
    assert torch.equal(t2.ema.shadow.view(torch.int32), t1.ema.shadow.view(torch.int32))
    assert t2.ema.scalars() == t1.ema.scalars() and t2.ema.cur_decay_value == t1.ema.get_decay(5)
    assert t2.opt_step == 3 and torch.equal(t2.exp_avg, t1.exp_avg)


def test_checkpoint_mismatches(tmp_path, monkeypatch):
    from pairwise_sample_optimization_amd import lora_io
    monkeypatch.setattr(lora_io, "load_lora_into_unet", lambda *a, **k: None)
    unet = _cpu_unet()
    with_ema, without = tmp_path / "with", tmp_path / "without"
    t_ema = _trainer(unet, 1)
    lora_io.save_state(t_ema, str(with_ema))
    t_plain = _trainer(_cpu_unet(), 2, with_ema=False)
    lora_io.save_state(t_plain, str(without))
    assert "ema" not in json.load(open(without / "pso_state.json"))
    assert not os.path.exists(without / lora_io.EMA_LORA_WEIGHT_NAME)
    # no EMA in the checkpoint, one in the trainer: KeyError saying so, nothing loaded
    t3 = _trainer(_cpu_unet(), 3)
    keep = (t3.ema.shadow.clone(), t3.exp_avg.clone())
    with pytest.raises(KeyError, match="no EMA state"):
        lora_io.load_state(t3, str(without))
    assert torch.equal(t3.ema.shadow, keep[0]) and torch.equal(t3.exp_avg, keep[1]) and t3.opt_step == 3
    # an EMA in the checkpoint, none in the trainer: the rest loads, with a warning
    t4 = _trainer(_cpu_unet(), 4, with_ema=False)
    t4.opt_step = 0
    with pytest.warns(UserWarning, match="EMA"):
        lora_io.load_state(t4, str(with_ema))
    assert t4.ema is None and t4.opt_step == 3 and torch.equal(t4.exp_avg, t_ema.exp_avg)
    # swapped in: neither direction
    t_ema.ema.swapped = True
    with pytest.raises(RuntimeError, match="swapped in"):
        lora_io.save_state(t_ema, str(tmp_path / "x"))
    with pytest.raises(RuntimeError, match="swapped in"):
        lora_io.load_state(t_ema, str(with_ema))


# ----------------------------------------------------------------------------------------------------------------------
# the C-ABI boundary
# ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from pairwise_sample_optimization_amd import _lib, kernels as K
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
    assert callable(K.ema_step) and callable(K.ema_swap)


def test_entries_reject_bad_arguments_before_any_launch():
    """Every call fails an argument check (PSO_ERR_ARG = 1 with a message that names the entry), so nothing is
    launched; the addresses are fakes that are never dereferenced.  Host-only on purpose, as tests/test_abi.py's
    argument probe is."""
    from pairwise_sample_optimization_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("argument checks are exercised where no launch can follow a regression (no GPU)")
    l = _lib.lib()
    A, B = 0x10000, 0x20000
    for n, s, p, omd in ((0, A, B, 0.5), (-3, A, B, 0.5), (8, None, B, 0.5), (8, A, None, 0.5), (8, A, B, -1e-3),
                         (8, A, B, 1.0001), (8, A, B, math.nan), (8, A, B, math.inf), (8, A + 2, B, 0.5)):
        rc = l.pso_ema_step(n, s, p, omd, None)
        assert rc == 1 and l.pso_last_error().decode().startswith("pso_ema_step: "), (n, s, p, omd, rc)
    for n, a, b in ((0, A, B), (-1, A, B), (8, None, B), (8, A, None), (8, A, A), (8, A, A + 16), (8, A + 16, A),
                    (8, A, B + 1)):
        rc = l.pso_ema_swap(n, a, b, None)
        assert rc == 1 and l.pso_last_error().decode().startswith("pso_ema_swap: "), (n, a, b, rc)


def test_kernel_wrappers_refuse_host_tensors():
    from pairwise_sample_optimization_amd import _lib, kernels as K
    with pytest.raises(_lib.PsoLibError, match="device tensors"):
        K.ema_step(torch.zeros(4), torch.zeros(4), 0.5)
    with pytest.raises(_lib.PsoLibError, match="device tensors"):
        K.ema_swap(torch.zeros(4), torch.ones(4))
