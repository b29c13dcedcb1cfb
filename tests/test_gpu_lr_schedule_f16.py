"""GPU cases of the learning-rate schedule under fp16 training (libpso_amd_f16.so, PSO_LIB=f16), where the loss scaler
decides which optimizer steps count: the schedule must follow the applied steps, on the host scaler (the host knows the
count) and on the device scaler (only the device does: pso_lr_schedule reads it there and the `_lr` optimizer entries
read the word it writes).

The module skips itself unless PSO_LIB=f16 (the element type is per process); tests/test_lr_schedule_f16_child.py runs
it in a fresh child process.  Shapes: tests/test_gpu_f16_amp.py::_trainer (UNetConfig.tiny(16), rank 8, one pair, one
accumulation window per epoch) with linear, w = 2, T = 6.  Overflow is an arithmetic inf (a loss scale of 2^30), never
a fault.

Bars.  Device scaler against host scaler: the scale is a power of two and both sides run the step at the same float32
lr, so the moments and the 8-bit state are bit-identical; the parameters differ only through the bias-correction
constants the device evaluates with its own powf / pow: 1e-6 * max|p|."""
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("PSO_LIB", "") != "f16",
                                 reason="fp16 library cases: run with PSO_LIB=f16 "
                                        "(tests/test_lr_schedule_f16_child.py does)")]

SCHEDULE = dict(lr_scheduler="linear", lr_warmup_steps=2, max_train_steps=6)
LAMBDA = [0.0, 0.5, 1.0, 0.75, 0.5, 0.25, 0.0]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _dev_scaler(**kw):
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    return DeviceLossScaler(device="cuda:0", **kw)


def _trainer(cuda, loss_scale, lr=1e-3, **kw):
    """tests/test_gpu_f16_amp.py::_trainer with the trainer's keyword arguments open."""
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, lr=lr,
                    loss_scale=loss_scale, **kw)
    g = _gen(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).half()
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).half()
    tid = compute_time_ids(128, 0, cuda)
    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    sb = tr.shuffle(buf, generator=_gen(100))
    return unet, tr, sb


def _state(tr):
    ts = dict(tr.adam8.tensors()) if tr.adam8 is not None else {"exp_avg": tr.exp_avg, "exp_avg_sq": tr.exp_avg_sq}
    return {k: v.clone() for k, v in ts.items()}


def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


@pytest.mark.parametrize("adam8", [False, True])
def test_schedule_follows_the_applied_steps_on_both_scalers(cuda, adam8):
    """Six epochs, the third at a loss scale of 2^30 (arithmetic inf: both scalers skip it).  The applied steps run at
    lambda(0), lambda(1), lambda(2), ... -- the skipped step does not advance the schedule.

    Both trainers run every epoch on their own weights with the optimizer held back; the optimizer steps then both
    consume the HOST trainer's epoch gradient.  AdamW's moments (and the 8-bit state) are a function of the gradient
    sequence alone, so they must be bit-identical throughout, while the parameters may drift apart by the
    bias-correction constants only.  Left on their own gradients the pair cannot stay bit-identical past the first
    steps: after a step at a non-zero lr the masters differ in their last bits (the 1e-6 bar), a few elements of the
    fp16 working copies then round the other way, and the next epoch's gradients are no longer the same bits
    (observed on an MI355X at the fifth epoch: exp_avg 1.8439e-04 against 1.8436e-04).  Where the weights are still
    the same bits -- the first two epochs: the first step runs at lr = 0 -- the two epoch gradients are compared too."""
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    u_d, tr_d, sb = _trainer(cuda, _dev_scaler(init_scale=1024.0), use_8bit_adam=adam8, **SCHEDULE)
    u_h, tr_h, _ = _trainer(cuda, 1024.0, use_8bit_adam=adam8, **SCHEDULE)
    assert isinstance(tr_d.scaler, DeviceLossScaler) and tr_d.lr_schedule is not None and tr_d.lr == tr_h.lr == 1e-3
    assert tr_d.last_lr is None and tr_h.last_lr is None
    applied, moved = 0, []
    for tr in (tr_d, tr_h):
        tr.auto_step = False
    for epoch in range(1, 7):
        if epoch == 3:
            for tr in (tr_d, tr_h):
                tr.scaler.scale = 2.0 ** 30
        before = (u_d.lora.master.clone(), u_h.lora.master.clone(), _state(tr_d))
        for tr in (tr_d, tr_h):
            tr.train_epoch(sb)
        g_d, g_h = u_d.lora.grad, u_h.lora.grad
        assert torch.isfinite(g_d).all().item() == torch.isfinite(g_h).all().item() == (epoch != 3)
        if epoch <= 2:
            assert g_h.abs().max().item() > 0 and torch.equal(g_d.view(torch.int32), g_h.view(torch.int32))
        g_d.copy_(g_h)
        for tr in (tr_d, tr_h):
            tr.optimizer_step()
        torch.cuda.synchronize()
        if epoch == 3:
            assert tr_d.scaler.skipped == tr_h.scaler.skipped == 1 and tr_d.scaler.scale == tr_h.scaler.scale == 2.0 ** 29
            assert torch.equal(u_d.lora.master, before[0]) and torch.equal(u_h.lora.master, before[1])
            for k, v in _state(tr_d).items():
                assert torch.equal(v, before[2][k]), k
            for tr in (tr_d, tr_h):
                tr.scaler.scale = 1024.0
        else:
            applied += 1
        assert tr_d.opt_step == tr_h.opt_step == applied
        want = _f32(1e-3 * LAMBDA[applied - 1])  # lambda(k), k = the steps applied before the last applied one
        assert tr_d.last_lr == tr_h.last_lr == want == tr_d.lr_schedule.lr32(applied - 1), (epoch, tr_d.last_lr, want)
        sd, sh = _state(tr_d), _state(tr_h)
        for k in sd:
            assert torch.equal(sd[k], sh[k]), (epoch, k)
        pm = u_h.lora.master.abs().max().item()
        d = (u_d.lora.master - u_h.lora.master).abs().max().item() / pm
        print(f"  adam8={adam8} epoch {epoch}: applied {applied} lr {tr_d.last_lr:.3e}  "
              f"{(u_d.lora.master != u_h.lora.master).sum().item()} of {u_h.lora.master.numel()} parameters differ, "
              f"max {d:.2e} of max|p|")
        assert d <= 1e-6
        moved.append(not torch.equal(u_h.lora.master, before[1]))
        assert u_d.lora.grad.abs().max().item() == 0.0 and u_h.lora.grad.abs().max().item() == 0.0
    # epoch 1 runs at lambda(0) = 0 and epoch 3 is skipped: neither moves the parameters; the others do
    assert moved == [False, True, False, True, True, True]
    assert tr_d.scaler.skipped == 1 and tr_d.opt_step == 5 and torch.isfinite(u_d.lora.master).all()
    assert torch.equal(u_d.lora.work.view(torch.int16), u_d.lora.master.half().view(torch.int16))


def test_prodigy_warms_up_under_the_device_scaler(cuda):
    """constant_with_warmup, w = 1: the first applied step runs at lr = 0 (Prodigy's k stays 0, the schedule moves on),
    the second at lr = 1."""
    unet, tr, sb = _trainer(cuda, _dev_scaler(init_scale=1024.0), lr=1.0, optimizer="prodigy",
                            lr_scheduler="constant_with_warmup", lr_warmup_steps=1)
    master0 = unet.lora.master.clone()
    tr.train_epoch(sb)
    sc = tr.prodigy.scalars()
    assert tr.opt_step == 1 and tr.last_lr == 0.0 and (sc["k"], sc["updated"], sc["skipped"]) == (0, 0, 0)
    assert torch.equal(unet.lora.master, master0) and tr.prodigy.exp_avg.abs().max().item() > 0
    tr.train_epoch(sb)
    sc = tr.prodigy.scalars()
    assert tr.opt_step == 2 and tr.last_lr == 1.0 and (sc["k"], sc["updated"]) == (1, 1)
    assert torch.isfinite(unet.lora.master).all() and not torch.equal(unet.lora.master, master0)


@pytest.mark.parametrize("adam8", [False, True])
def test_optimizer_step_with_a_schedule_does_not_sync(cuda, adam8):
    """tests/test_gpu_f16_amp.py::test_optimizer_step_does_not_sync with a schedule set: the lr is evaluated and read
    on the device.  Two steps, so that the second runs at a non-zero lr."""
    unet, tr, sb = _trainer(cuda, _dev_scaler(init_scale=1024.0), use_8bit_adam=adam8, **SCHEDULE)
    tr.auto_step = False
    tr.train_epoch(sb)
    grad = unet.lora.grad.clone()
    torch.cuda.synchronize()
    probe = torch.ones(1, device=cuda)
    master0 = unet.lora.master.clone()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            tr.optimizer_step()
            unet.lora.grad.copy_(grad)
            tr.optimizer_step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
    assert tr.opt_step == 2 and tr.last_lr == _f32(0.5e-3) and not torch.equal(unet.lora.master, master0)
