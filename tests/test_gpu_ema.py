"""GPU cases of the EMA of the trained weights on the default (bf16) library: pso_ema_step against tests/ema_ref.py and
pso_ema_swap, bit for bit; 64-bit indexing; the trainers' optimizer step with use_ema; DoRA; average_parameters();
checkpoints.  The fp16 / device-scaler case runs under PSO_LIB=f16 (tests/test_gpu_ema_f16.py).

Bounds.  The element update is three fp32 operations, each correctly rounded on the device as in numpy: bit equality
with the restatement, for every size, alignment and factor.  A swap moves bits: equality.  EMA reads the master and
writes only its shadow: the training of a use_ema trainer is bit-identical to one without."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 2048 * 5 + 1003]
OMDS = [np.float32(0.0), np.float32(1.0), np.float32(1 - 0.9999), np.float32(9 / 11)]
SENT = 123.25
DECAYS = [0.0, 2 / 11, 3 / 12, 4 / 13, 5 / 14]


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """Building a UNet draws from torch's global generators before init_weights() overwrites the values: leave both
    streams as they were, so later test files that read them unseeded see the numbers they saw before."""
    with torch.random.fork_rng(devices=[0] if torch.cuda.is_available() else []):
        yield


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _view(cuda, n, misaligned, gen=None):
    """(buffer, view): n floats inside a sentinel-filled buffer, 16-B aligned or offset by one float from that, with
    sentinel floats directly before and after."""
    buf = torch.full((n + 8,), SENT, device=cuda)
    lo = 5 if misaligned else 4
    v = buf[lo:lo + n]
    assert v.data_ptr() % 16 == (4 if misaligned else 0)
    if gen is not None:
        v.copy_(torch.randn(n, device=cuda, generator=gen))
    return buf, v, lo


def _sentinels_intact(buf, lo, n):
    return bool((buf[:lo] == SENT).all().item() and (buf[lo + n:] == SENT).all().item())


# ----------------------------------------------------------------------------------------------------------------------
# 1. pso_ema_step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_ema_step_is_the_restatement(cuda, n, misaligned):
    from pairwise_sample_optimization_amd import kernels as K
    for j, omd in enumerate(OMDS):
        g = _gen(1000 * j + n)
        sbuf, s, lo = _view(cuda, n, misaligned, g)
        pbuf, p, _ = _view(cuda, n, misaligned, g)
        s0, p0 = s.cpu().numpy(), p.cpu().numpy()
        K.ema_step(s, p, float(omd))
        want = ema_ref.ema_update(s0, p0, omd)
        got = s.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, misaligned, omd)
        assert np.array_equal(p.cpu().numpy().view(np.int32), p0.view(np.int32))  # the parameters are only read
        assert _sentinels_intact(sbuf, lo, n) and _sentinels_intact(pbuf, lo, n)
        if omd == 0.0:
            assert np.array_equal(got.view(np.int32), s0.view(np.int32))  # bits untouched
        elif n >= 255:
            assert not np.array_equal(got, s0)


def test_ema_step_argument_errors_write_nothing(cuda):
    from pairwise_sample_optimization_amd import _lib, kernels as K
    l = _lib.lib()
    s = torch.full((64,), 2.0, device=cuda)
    p = torch.full((64,), 1.0, device=cuda)
    sp = _lib.stream_ptr()
    calls = [(0, s.data_ptr(), p.data_ptr(), 0.5), (-1, s.data_ptr(), p.data_ptr(), 0.5),
             (64, None, p.data_ptr(), 0.5), (64, s.data_ptr(), None, 0.5), (64, s.data_ptr(), p.data_ptr(), -0.25),
             (64, s.data_ptr(), p.data_ptr(), 1.5), (64, s.data_ptr(), p.data_ptr(), float("nan")),
             (64, s.data_ptr(), p.data_ptr(), float("inf"))]
    for n, a, b, omd in calls:
        assert l.pso_ema_step(n, a, b, omd, sp) == 1, (n, a, b, omd)  # PSO_ERR_ARG
        assert l.pso_last_error().decode().startswith("pso_ema_step: ")
    with pytest.raises(_lib.PsoLibError, match="one_minus_decay"):
        K.ema_step(s, p, 2.0)
    with pytest.raises(_lib.PsoLibError, match="sizes differ"):
        K.ema_step(s, p[:32], 0.5)
    with pytest.raises(_lib.PsoLibError, match="float32"):
        K.ema_step(s, p.double(), 0.5)
    torch.cuda.synchronize()
    assert (s == 2.0).all().item() and (p == 1.0).all().item()


# ----------------------------------------------------------------------------------------------------------------------
# 2. pso_ema_swap
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_is_exact_and_its_own_inverse(cuda, n, misaligned):
    from pairwise_sample_optimization_amd import kernels as K
    g = _gen(n)
    abuf, a, lo = _view(cuda, n, misaligned, g)
    bbuf, b, _ = _view(cuda, n, misaligned, g)
    if n >= 4:  # bit patterns a float operation would not carry through: a signalling nan, -0, a denormal
        a[:3].view(torch.int32).copy_(torch.tensor([0x7FA00001, -2 ** 31, 1], dtype=torch.int32))
    a0, b0 = _bits(a).clone(), _bits(b).clone()
    K.ema_swap(a, b)
    assert torch.equal(_bits(a), b0) and torch.equal(_bits(b), a0)
    assert _sentinels_intact(abuf, lo, n) and _sentinels_intact(bbuf, lo, n)
    K.ema_swap(a, b)
    assert torch.equal(_bits(a), a0) and torch.equal(_bits(b), b0)
    assert _sentinels_intact(abuf, lo, n) and _sentinels_intact(bbuf, lo, n)


def test_ema_swap_argument_errors_write_nothing(cuda):
    from pairwise_sample_optimization_amd import _lib, kernels as K
    l = _lib.lib()
    a = torch.full((64,), 2.0, device=cuda)
    b = torch.full((64,), 1.0, device=cuda)
    sp = _lib.stream_ptr()
    for n, x, y in ((0, a.data_ptr(), b.data_ptr()), (-5, a.data_ptr(), b.data_ptr()), (64, None, b.data_ptr()),
                    (64, a.data_ptr(), None), (64, a.data_ptr(), a.data_ptr()), (32, a.data_ptr(), a.data_ptr() + 64)):
        assert l.pso_ema_swap(n, x, y, sp) == 1, (n, x, y)  # PSO_ERR_ARG
        assert l.pso_last_error().decode().startswith("pso_ema_swap: ")
    with pytest.raises(_lib.PsoLibError, match="same buffer"):
        K.ema_swap(a, a)
    with pytest.raises(_lib.PsoLibError, match="sizes differ"):
        K.ema_swap(a, b[:8])
    torch.cuda.synchronize()
    assert (a == 2.0).all().item() and (b == 1.0).all().item()


# ----------------------------------------------------------------------------------------------------------------------
# 3. 64-bit indexing
# ----------------------------------------------------------------------------------------------------------------------
def test_indices_past_two_to_the_31(cuda):
    """n = 2^31 + 5 (the full-UNet master has 2.57e9 elements): two 8.6 GB buffers of constants; the head, the 16
    elements around index 2^31 and the tail are verified.  s = 3, p = 1, factor 1/2: t = 2, u = 1, s = 2, exactly."""
    from pairwise_sample_optimization_amd import kernels as K
    n = 2 ** 31 + 5
    free, _ = torch.cuda.mem_get_info()
    if free < 40e9:
        pytest.skip(f"needs 40 GB of free device memory, {free / 1e9:.1f} GB are free")
    s = torch.full((n,), 3.0, device=cuda)
    p = torch.full((n,), 1.0, device=cuda)
    slices = (slice(0, 16), slice(2 ** 31 - 8, 2 ** 31 + 8), slice(n - 16, n))
    K.ema_step(s, p, 0.5)
    for sl in slices:
        assert (s[sl] == 2.0).all().item() and (p[sl] == 1.0).all().item(), sl
    K.ema_swap(s, p)
    for sl in slices:
        assert (s[sl] == 1.0).all().item() and (p[sl] == 2.0).all().item(), sl
    del s, p
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# 4. the trainers
# ----------------------------------------------------------------------------------------------------------------------
def _unet(cuda, dora=False, adapter=True):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    if adapter:
        st = unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=dora), allow_dora=True)
        st.init_gaussian(seed=1, b_std=0.05)
        if dora:
            st.init_magnitudes()
    unet.prepare()
    return unet


def _fill_grad(unet, step):
    """tests/test_gpu_lr_schedule.py::_fill_grad: fixed random values into the flat gradient (3 x N(0, 1): clips)."""
    unet.lora.grad.copy_(torch.randn(unet.lora.grad.shape, device=unet.lora.grad.device, generator=_gen(50 + step)) * 3)


OPTIMIZERS = {"adamw": dict(lr=1e-3, weight_decay=1e-2),
              "adamw8bit": dict(lr=1e-3, weight_decay=1e-2, use_8bit_adam=True),
              "prodigy": dict(lr=1.0, weight_decay=1e-2, optimizer="prodigy", prodigy_d0=1e-3, betas=(0.9, 0.99))}


def _trainer(cuda, opt="adamw", use_ema=True, dora=False, **kw):
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    unet = _unet(cuda, dora=dora)
    ema = dict(use_ema=True, ema_decay=0.9) if use_ema else {}
    return unet, PSOTrainer(unet, mode="turbo", num_steps=2, **OPTIMIZERS[opt], **ema, **kw)


def _step_and_check(unet, tr, step, want_decay):
    """One optimizer step on the gradient of `step`; the shadow against the restatement applied to the previous shadow
    and the new master."""
    prev = tr.ema.shadow.cpu().numpy()
    _fill_grad(unet, step)
    tr.optimizer_step()
    assert tr.ema.optimization_step == step and tr.ema.cur_decay_value == want_decay
    want = ema_ref.ema_update(prev, unet.lora.master.cpu().numpy(), ema_ref.one_minus_decay32(want_decay))
    got = tr.ema.shadow.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), step
    return prev, got


@pytest.mark.parametrize("opt", sorted(OPTIMIZERS))
def test_trainer_updates_the_shadow_and_trains_the_same_bits(cuda, opt):
    from pairwise_sample_optimization_amd.ema import EMAModel
    ua, tra = _trainer(cuda, opt)
    ub, trb = _trainer(cuda, opt, use_ema=False)
    assert isinstance(tra.ema, EMAModel) and trb.ema is None
    assert torch.equal(_bits(tra.ema.shadow), _bits(ua.lora.master)) and tra.ema.cur_decay_value is None
    m0 = ua.lora.master.clone()
    for step in range(1, 6):
        prev, got = _step_and_check(ua, tra, step, DECAYS[step - 1])
        _fill_grad(ub, step)
        trb.optimizer_step()
        assert tra.opt_step == trb.opt_step == step
        # EMA changes nothing of the training
        assert torch.equal(_bits(ua.lora.master), _bits(ub.lora.master)), step
        assert torch.equal(ua.lora.work.view(torch.int16), ub.lora.work.view(torch.int16))
        if step >= 2:  # decay > 0: the shadow lags behind the master
            assert not np.array_equal(got, ua.lora.master.cpu().numpy()) and not np.array_equal(got, prev)
    assert not torch.equal(ua.lora.master, m0) and tra.ema.decay == 0.9


def test_dreambooth_trainer_steps_the_ema(cuda):
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    unet = _unet(cuda)
    tr = DreamBoothPSOTrainer(unet, None, learning_rate=1e-3, use_ema=True, ema_decay=0.9, ema_update_after_step=1)
    assert DreamBoothPSOTrainer(unet, None).ema is None
    for step, want in zip(range(1, 5), [0.0, 0.0, 2 / 11, 3 / 12]):
        _step_and_check(unet, tr, step, want)


# ----------------------------------------------------------------------------------------------------------------------
# 5. DoRA
# ----------------------------------------------------------------------------------------------------------------------
def test_dora_magnitudes_are_averaged_with_the_rest(cuda):
    unet, tr = _trainer(cuda, "adamw", dora=True)
    st = unet.lora
    assert st.dora
    mask = torch.zeros(st.master.numel(), dtype=torch.bool, device=cuda)
    base = st.master.storage_offset()
    for name in st.adapter_names():
        m = st.magnitude_view(st.master, name)
        o = m.storage_offset() - base
        mask[o:o + m.numel()] = True
    assert 0 < int(mask.sum()) < mask.numel()
    shadow0 = tr.ema.shadow.clone()
    for step in range(1, 4):
        _step_and_check(unet, tr, step, DECAYS[step - 1])
    moved = tr.ema.shadow != shadow0
    assert moved[mask].float().mean().item() > 0.9 and moved[~mask].float().mean().item() > 0.9
    # the magnitude segments of the shadow lag the master's like every other segment
    assert not torch.equal(tr.ema.shadow[mask], st.master[mask])
    sd = tr.ema.state_dict_peft()
    name = next(iter(st.adapter_names()))
    assert torch.equal(sd[f"{name}.lora_magnitude_vector.weight"], st.magnitude_view(tr.ema.shadow, name))


# ----------------------------------------------------------------------------------------------------------------------
# 6. average_parameters()
# ----------------------------------------------------------------------------------------------------------------------
def _inputs(cuda, cfg):
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    g = _gen(3)
    x = K.cast_f32_bf16(torch.randn(2, 16, 16, 4, device=cuda, generator=g))
    t = torch.tensor([999.0, 499.0], device=cuda)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, device=cuda, generator=g).bfloat16()
    pooled = torch.randn(2, cfg.text_embed_dim, device=cuda, generator=g).bfloat16()
    tid = compute_time_ids(128, 0, cuda).repeat(2, 1)
    return x, t, enc, pooled, tid


def _eps(unet, inp):
    with torch.no_grad():
        return unet.forward_nhwc(*inp, save=False)[0].clone()


@pytest.mark.parametrize("dora", [False, True])
def test_average_parameters(cuda, dora):
    unet, tr = _trainer(cuda, "adamw", dora=dora)
    for step in range(1, 4):
        _fill_grad(unet, step)
        tr.optimizer_step()
    ema, st = tr.ema, unet.lora
    inp = _inputs(cuda, unet.cfg)
    keep = dict(master=_bits(st.master).clone(), shadow=_bits(ema.shadow).clone(),
                work=st.work.view(torch.int16).clone())
    assert not torch.equal(keep["master"], keep["shadow"])
    eps_live = _eps(unet, inp)
    twin = _unet(cuda, dora=dora)  # an identically built UNet whose adapter is loaded from the shadow
    twin.lora.load_peft(ema.state_dict_peft())
    assert torch.equal(_bits(twin.lora.master), keep["shadow"])
    eps_twin = _eps(twin, inp)
    twin.fuse_lora()
    eps_twin_fused = _eps(twin, inp)
    assert not torch.equal(eps_twin, eps_live)  # the averaged weights compute something else
    version = st.version
    with ema.average_parameters() as inside:
        assert inside is ema and ema.swapped and st.version > version
        assert torch.equal(_bits(st.master), keep["shadow"]) and torch.equal(_bits(ema.shadow), keep["master"])
        assert torch.equal(_eps(unet, inp).view(torch.int16), eps_twin.view(torch.int16))
        unet.fuse_lora()
        assert torch.equal(_eps(unet, inp).view(torch.int16), eps_twin_fused.view(torch.int16))
        unet.unfuse_lora()
        with pytest.raises(RuntimeError, match="micro_step while the EMA weights"):
            tr.micro_step(None)
        with pytest.raises(RuntimeError, match="optimizer_step while the EMA weights"):
            tr.optimizer_step()
        with pytest.raises(RuntimeError, match="already swapped in"):
            ema.copy_to()
        with pytest.raises(RuntimeError, match="swapped in"):
            with ema.average_parameters():
                pass
        with pytest.raises(RuntimeError, match="swapped in"):
            ema.step()
        assert ema.swapped and ema.optimization_step == 3 and tr.opt_step == 3
    assert not ema.swapped
    assert torch.equal(_bits(st.master), keep["master"]) and torch.equal(_bits(ema.shadow), keep["shadow"])
    assert torch.equal(st.work.view(torch.int16), keep["work"])
    assert torch.equal(_eps(unet, inp).view(torch.int16), eps_live.view(torch.int16))
    # diffusers' names do the same, and training goes on afterwards
    ema.store()
    ema.copy_to()
    assert torch.equal(_bits(st.master), keep["shadow"])
    ema.restore()
    assert torch.equal(_bits(st.master), keep["master"]) and torch.equal(_bits(ema.shadow), keep["shadow"])
    with pytest.raises(RuntimeError, match="restore"):
        ema.restore()
    _fill_grad(unet, 4)
    tr.optimizer_step()
    assert ema.optimization_step == 4 and ema.cur_decay_value == DECAYS[3]


# ----------------------------------------------------------------------------------------------------------------------
# 7. checkpoints
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dora", [False, True])
def test_checkpoint_resumes_bit_for_bit(cuda, tmp_path, dora):
    from pairwise_sample_optimization_amd import lora_io
    ua, tra = _trainer(cuda, "adamw", dora=dora)
    for step in range(1, 4):
        _fill_grad(ua, step)
        tra.optimizer_step()
    lora_io.save_state(tra, str(tmp_path))
    shadow3 = _bits(tra.ema.shadow).clone()
    for step in range(4, 6):
        _fill_grad(ua, step)
        tra.optimizer_step()
    ub, trb = _trainer(cuda, "adamw", dora=dora)
    lora_io.load_state(trb, str(tmp_path))
    assert trb.opt_step == 3 and trb.ema.optimization_step == 3 and trb.ema.cur_decay_value == DECAYS[2]
    assert torch.equal(_bits(trb.ema.shadow), shadow3)
    for step in range(4, 6):
        _fill_grad(ub, step)
        trb.optimizer_step()
    assert trb.ema.optimization_step == tra.ema.optimization_step == 5 and trb.opt_step == tra.opt_step == 5
    assert torch.equal(_bits(ub.lora.master), _bits(ua.lora.master))
    assert torch.equal(_bits(trb.ema.shadow), _bits(tra.ema.shadow))
    assert not torch.equal(_bits(tra.ema.shadow), shadow3)
    # the EMA LoRA file loads like any adapter and reproduces the shadow as saved
    plain = _unet(cuda, dora=dora)
    lora_io.load_lora_weights(plain, str(tmp_path), weight_name=lora_io.EMA_LORA_WEIGHT_NAME)
    assert torch.equal(_bits(plain.lora.master), shadow3)
    lora_io.load_lora_weights(plain, str(tmp_path))
    assert not torch.equal(_bits(plain.lora.master), shadow3)
    # the mismatch rules on the device
    uc, trc = _trainer(cuda, "adamw", use_ema=False, dora=dora)
    with pytest.warns(UserWarning, match="EMA"):
        lora_io.load_state(trc, str(tmp_path))
    assert trc.ema is None and trc.opt_step == 3
    lora_io.save_state(trc, str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="no EMA state"):
        lora_io.load_state(trb, str(tmp_path / "plain"))
