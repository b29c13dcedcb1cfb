"""CPU checks of the learning-rate schedule: lr_schedule.LrSchedule against the lambdas of
transformers.optimization.get_scheduler (the six kinds diffusers' get_scheduler offers the DreamBooth script; diffusers
itself is not installed here), the world-size cancellation, the argument errors, the
DreamBooth front door and the checkpoint entry; and the C-ABI boundary of the new entries in all three libraries."""
import json
import math
import os
import re
import subprocess
import warnings
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pairwise_sample_optimization_amd")
KINDS = ["constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial"]
SETTINGS = [(3, 12, 2, 2.0), (0, 5, 1, 1.0), (4, 5, 3, 0.5)]  # (warm-up, total, cycles, power)
BASE_LR = 2e-4
NEW = ["pso_lr_schedule", "pso_adamw_step", "pso_adamw8bit_step", "pso_prodigy_step_lr"]


def _oracle(kind, w, T, cycles, power, steps):
    """lambda(0 .. steps - 1) of transformers' scheduler, built as diffusers' get_scheduler builds its own: num_cycles
    goes to cosine_with_restarts only and power to polynomial only."""
    from transformers.optimization import get_scheduler
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=BASE_LR)
    extra = {"cosine_with_restarts": {"num_cycles": cycles}, "polynomial": {"power": power}}.get(kind)
    sch = get_scheduler(kind, opt, num_warmup_steps=w, num_training_steps=T, scheduler_specific_kwargs=extra)
    return [sch.lr_lambdas[0](k) for k in range(steps)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "w%d-T%d-c%d-p%g" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_multiplier_matches_the_transformers_lambdas(kind, setting):
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    w, T, cycles, power = setting
    sched = LrSchedule(kind, BASE_LR, w, T, cycles, power)
    want = _oracle(kind, w, T, cycles, power, T + 4)
    got = [sched.multiplier(k) for k in range(T + 4)]
    assert all(isinstance(x, float) for x in got)
    worst = max(abs(a - b) for a, b in zip(got, want))
    print(f"  {kind} {setting}: max |diff| {worst:.2e}")
    assert worst <= 1e-12, (got, want)
    assert [sched.lr(k) for k in range(T + 4)] == [BASE_LR * x for x in got]
    if kind == "constant":
        assert got == [1.0] * (T + 4)  # ignores the warm-up
    elif w:
        assert got[0] == 0.0 and got[1] == 1.0 / w  # the first step runs at lambda(0) = 0


def test_the_oracle_shows_the_two_oddities_the_schedule_keeps():
    """cosine rises again after T (num_cycles = 0.5 is a half wave, not clamped); polynomial sits at lr_end / base_lr."""
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    cos = LrSchedule("cosine", BASE_LR, 3, 12)
    assert cos.multiplier(12) <= 1e-30 and cos.multiplier(15) > cos.multiplier(13) > 0.0
    assert cos.multiplier(15) == _oracle("cosine", 3, 12, 1, 1.0, 16)[15]
    pol = LrSchedule("polynomial", BASE_LR, 3, 12, power=2.0)
    assert pol.multiplier(13) == pol.multiplier(40) == 1e-7 / BASE_LR == _oracle("polynomial", 3, 12, 1, 2.0, 14)[13]
    rest = LrSchedule("cosine_with_restarts", BASE_LR, 3, 12, num_cycles=2)
    assert rest.multiplier(12) == 0.0 and rest.multiplier(20) == 0.0  # p >= 1


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_world_size_cancels(kind, W):
    """accelerate's way: warm-up and total multiplied by the world size W, the scheduler stepped W times per optimizer
    step, so optimizer step k sees lambda(k W; w W, T W).  It equals multiplier(k) with the unscaled counts."""
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    for w, T, cycles, power in SETTINGS:
        mine = LrSchedule(kind, BASE_LR, w, T, cycles, power)
        scaled = _oracle(kind, w * W, T * W, cycles, power, (T + 4) * W)
        for k in range(T + 4):
            assert abs(scaled[k * W] - mine.multiplier(k)) <= 1e-12, (kind, W, k)


def test_argument_errors():
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule, make_lr_schedule
    for name in ("piecewise_constant", "exponential", ""):
        with pytest.raises(ValueError, match="lr_scheduler"):
            LrSchedule(name, BASE_LR, 0, 10)
        with pytest.raises(ValueError, match="lr_scheduler"):
            make_lr_schedule(name, BASE_LR, 0, 10)
    for kind in ("linear", "cosine", "cosine_with_restarts", "polynomial"):
        with pytest.raises(ValueError, match="max_train_steps"):
            LrSchedule(kind, BASE_LR, 3)
    LrSchedule("constant_with_warmup", BASE_LR, 3)  # needs no total
    for lr in (1e-7, 5e-8):
        with pytest.raises(ValueError, match="lr_end"):
            LrSchedule("polynomial", lr, 0, 10)
    with pytest.raises(ValueError, match="max_train_steps"):
        LrSchedule("polynomial", BASE_LR, 5, 5)  # diffusers would divide by zero at step 5
    assert make_lr_schedule("constant", BASE_LR, 500) is None
    assert make_lr_schedule("linear", BASE_LR, 2, 6).state_dict() == LrSchedule("linear", BASE_LR, 2, 6).state_dict()


def test_lr32_is_the_float32_rounding_and_state_dict_round_trips():
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    s = LrSchedule("cosine_with_restarts", 3e-4, 3, 12, num_cycles=2)
    for k in range(16):
        assert s.lr32(k) == torch.tensor(s.lr(k), dtype=torch.float64).to(torch.float32).item()
    sd = s.state_dict()
    assert sd == {"kind": "cosine_with_restarts", "base_lr": 3e-4, "num_warmup_steps": 3, "num_training_steps": 12,
                  "num_cycles": 2, "power": 1.0}
    other = LrSchedule("constant_with_warmup", 1.0, 1)
    other.load_state_dict(json.loads(json.dumps(sd)))
    assert other.state_dict() == sd and [other.lr(k) for k in range(16)] == [s.lr(k) for k in range(16)]
    with pytest.raises(ValueError, match="lr_scheduler"):
        other.load_state_dict(dict(sd, kind="piecewise_constant"))


def _unet():
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    return unet


def _args(**kw):
    """personalization/scripts/pso_dog.sh as the script's namespace, the schedule flags left to the caller."""
    base = dict(loss_type="pso_db", beta_pso=5, neg_defactor=0.1, prior_loss_weight=0.5, distill_train_timesteps=4,
                learning_rate=2e-4, gradient_accumulation_steps=4, mixed_precision="fp16", optimizer="AdamW",
                do_edm_style_training=True)
    base.update(kw)
    return SimpleNamespace(**base)


def test_from_args_builds_the_schedule_on_request_only():
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    unet = _unet()
    # the script's own argparse defaults: constant with a warm-up of 500 that the constant kind ignores
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        DreamBoothPSOTrainer.from_args(unet, None, _args())
    tr = DreamBoothPSOTrainer.from_args(unet, None, _args(), allow_lr_schedule=True)
    assert tr.lr_schedule is None and tr.lr_word is None and tr.lr == 2e-4 and tr.last_lr is None
    tr = DreamBoothPSOTrainer.from_args(unet, None, _args(lr_scheduler="constant", lr_warmup_steps=500),
                                        allow_lr_schedule=True)
    assert tr.lr_schedule is None
    args = _args(lr_scheduler="cosine", lr_warmup_steps=500, max_train_steps=1600)
    with pytest.raises(ValueError, match="lr_scheduler"):  # refused as it always was
        DreamBoothPSOTrainer.from_args(unet, None, args)
    tr = DreamBoothPSOTrainer.from_args(unet, None, args, allow_lr_schedule=True)
    assert isinstance(tr.lr_schedule, LrSchedule) and tr.lr == 2e-4  # trainer.lr stays the base rate
    assert tr.lr_schedule.state_dict() == LrSchedule("cosine", 2e-4, 500, 1600).state_dict()
    assert tr.lr_word.shape == (1,) and tr.lr_word.dtype == torch.float32
    assert tr.lr_schedule.lr(0) == 0.0 and tr.lr_schedule.lr(250) == 1e-4 and tr.lr_schedule.lr(500) == 2e-4
    assert abs(tr.lr_schedule.lr(1050) - 1e-4) < 1e-18 and tr.opt_step == 0
    # no lr_warmup_steps in the namespace: the script's default of 500
    tr = DreamBoothPSOTrainer.from_args(unet, None, _args(lr_scheduler="linear", max_train_steps=1000,
                                                          lr_num_cycles=3, lr_power=2.0), allow_lr_schedule=True)
    assert tr.lr_schedule.state_dict() == LrSchedule("linear", 2e-4, 500, 1000, 3, 2.0).state_dict()
    with pytest.raises(ValueError, match="max_train_steps"):
        DreamBoothPSOTrainer.from_args(unet, None, _args(lr_scheduler="linear"), allow_lr_schedule=True)
    with pytest.raises(ValueError, match="lr_scheduler"):
        DreamBoothPSOTrainer.from_args(unet, None, _args(lr_scheduler="piecewise_constant"), allow_lr_schedule=True)


def test_both_trainers_take_the_schedule_arguments():
    from pairwise_sample_optimization_amd.config import config_sdxl_turbo_dpo
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _unet()
    tr = DreamBoothPSOTrainer(unet, None, lr_scheduler="polynomial", lr_warmup_steps=2, max_train_steps=9, lr_power=2.0)
    assert tr.lr_schedule.state_dict()["power"] == 2.0 and tr.lr == 2e-4
    assert DreamBoothPSOTrainer(unet, None).lr_schedule is None
    cfg = config_sdxl_turbo_dpo.get_config()
    tr = PSOTrainer.from_config(unet, cfg)
    assert tr.lr_schedule is None and tr.lr_word is None  # an absent key counts as constant
    cfg.train["lr_scheduler"], cfg.train["lr_warmup_steps"], cfg.train["max_train_steps"] = "cosine_with_restarts", 10, 100
    cfg.train["lr_num_cycles"] = 4
    tr = PSOTrainer.from_config(unet, cfg)
    sd = tr.lr_schedule.state_dict()
    assert (sd["kind"], sd["num_warmup_steps"], sd["num_training_steps"], sd["num_cycles"], sd["base_lr"]) == \
        ("cosine_with_restarts", 10, 100, 4, float(cfg.train.learning_rate))
    assert tr.lr == cfg.train.learning_rate
    tr.opt_step = 11  # host step count: last_lr is lr(opt_step - 1) as float32
    assert tr.last_lr == tr.lr_schedule.lr32(10)
    with pytest.raises(ValueError, match="lr_scheduler"):
        PSOTrainer(unet, lr_scheduler="piecewise_constant")


def _fake_trainer(sched, opt_step=3):
    n = 64
    lora = SimpleNamespace(r=8, state_dict_peft=lambda: {"a.attn1.to_q.lora_A.weight": torch.ones(8, 4),
                                                         "a.attn1.to_q.lora_B.weight": torch.zeros(4, 8)})
    return SimpleNamespace(unet=SimpleNamespace(lora=lora), exp_avg=torch.rand(n), exp_avg_sq=torch.rand(n),
                           opt_step=opt_step, n_micro=12, scaler=None, lr_schedule=sched,
                           lr_word=None if sched is None else torch.zeros(1))


def test_checkpoint_carries_the_schedule(tmp_path, monkeypatch):
    from pairwise_sample_optimization_amd import lora_io
    from pairwise_sample_optimization_amd.lr_schedule import LrSchedule
    monkeypatch.setattr(lora_io, "load_lora_into_unet", lambda *a, **k: None)  # the LoRA file is not tested here
    src = LrSchedule("linear", 1e-3, 2, 6)
    t1 = _fake_trainer(src)
    lora_io.save_state(t1, str(tmp_path))
    meta = json.load(open(tmp_path / "pso_state.json"))
    assert meta["lr_schedule"] == src.state_dict() and meta["opt_step"] == 3 and "loss_scaler" not in meta
    t2 = _fake_trainer(LrSchedule("linear", 1e-3, 2, 6), opt_step=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the same schedule: no warning
        lora_io.load_state(t2, str(tmp_path))
    assert t2.opt_step == 3 and t2.lr_schedule.state_dict() == src.state_dict()
    assert t2.lr_word.item() == src.lr32(2)  # the position is opt_step: the word holds the last applied step's lr
    t3 = _fake_trainer(LrSchedule("cosine", 1e-3, 2, 6), opt_step=0)
    with pytest.warns(UserWarning, match="schedule"):
        lora_io.load_state(t3, str(tmp_path))
    assert t3.lr_schedule.kind == "cosine" and t3.opt_step == 3  # the trainer's schedule wins
    t4 = _fake_trainer(None, opt_step=0)
    with pytest.warns(UserWarning, match="constant rate"):
        lora_io.load_state(t4, str(tmp_path))
    assert t4.lr_schedule is None and t4.opt_step == 3
    # a trainer without a schedule writes no key, and a checkpoint without the key loads without a word
    lora_io.save_state(t4, str(tmp_path))
    assert "lr_schedule" not in json.load(open(tmp_path / "pso_state.json"))
    t5 = _fake_trainer(LrSchedule("cosine", 1e-3, 2, 6), opt_step=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lora_io.load_state(t5, str(tmp_path))
    assert t5.opt_step == 3 and t5.lr_schedule.kind == "cosine"


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
    assert _lib.lib().pso_abi_version() == 2
    kinds = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define PSO_LR_(\w+) (\d+)", h)}
    assert kinds == _lib.LR_KINDS and sorted(kinds) == sorted(KINDS)


def test_pso_lr_schedule_rejects_bad_arguments_before_any_launch():
    """Every call fails an argument check (PSO_ERR_ARG = 1 with a message that names the entry), so nothing is
    launched; the output address is a fake that is never dereferenced.  Host-only on purpose, as
    tests/test_abi.py's argument probe is."""
    from pairwise_sample_optimization_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("argument checks are exercised where no launch can follow a regression (no GPU)")
    l = _lib.lib()
    OUT = 0x10000
    bad = [dict(kind=6), dict(kind=-1), dict(out=None), dict(base_lr=0.0), dict(base_lr=-1.0), dict(step=0),
           dict(kind=5, base_lr=1e-7), dict(kind=5, warmup=12, total=12), dict(warmup=-1), dict(out=OUT + 2)]
    for kw in bad:
        a = dict(kind=2, base_lr=1e-3, warmup=3, total=12, cycles=1, power=1.0, amp=None, step=1, out=OUT)
        a.update(kw)
        rc = l.pso_lr_schedule(a["kind"], a["base_lr"], a["warmup"], a["total"], a["cycles"], a["power"], a["amp"],
                               a["step"], a["out"], None)
        assert rc == 1 and l.pso_last_error().decode().startswith("pso_lr_schedule: "), (kw, rc)
    rc = l.pso_prodigy_step_lr(8, OUT, OUT, OUT, OUT, OUT, OUT, OUT, None, 0.9, 0.99, 0.99, 1e-8, 0.0, 1, 1.0,
                               math.inf, 1.0, None, None, OUT, 1 << 20, None)
    assert rc == 1 and "lr_dev" in l.pso_last_error().decode()
    # the unified step entries: (lr_dev, step, amp_state) of pso_adamw_step, then desc = NULL with zero_grad = 1
    for lr_dev, step, amp in ((None, 0, None), (OUT + 2, 1, None), (None, 1, OUT + 2)):
        rc = l.pso_adamw_step(8, OUT, OUT, OUT, OUT, 1e-3, lr_dev, 0.9, 0.99, 1e-8, 0.0, step, 1.0, None, amp, None)
        assert rc == 1 and l.pso_last_error().decode().startswith("pso_adamw_step: "), (lr_dev, step, amp, rc)
    rc = l.pso_adamw8bit_step(8, 1, None, OUT, None, OUT, 1, OUT, OUT, OUT, OUT, None, None, 1e-3, None, 0.9, 0.99,
                              1e-8, 0.0, 1, 1.0, None, None, None)
    assert rc == 1 and l.pso_last_error().decode().startswith("pso_adamw8bit_step: ")
