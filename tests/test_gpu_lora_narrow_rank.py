"""LoRA ranks below 8 (diffusers' default rank 4) on the GPU: the padded working copies (pso_lora_pack), the gradient
fold (pso_lora_grad_fold) and everything built on them -- forward / backward against the zero-padded rank-8 adapter
(bit for bit) and against the fp32 oracle, the side stream, hipGraph replay, the optimizer on peft's tensors, the
overlapped gradient sync, checkpoints and the DreamBooth micro-step.

Runs on the loaded library's element type (bf16, or fp16 in the PSO_LIB=f16 child of
tests/test_lora_narrow_rank_f16.py); sizes are the suite's tiny ones (UNetConfig.tiny(16), B = 2)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pairwise_sample_optimization_amd import _lib

pytestmark = pytest.mark.gpu

ELEM = _lib.ELEM_DTYPE
F16 = _lib.F16
HERE = os.path.dirname(os.path.abspath(__file__))
SB_KEYS = ("x", "x_next", "unet_in", "enc", "pooled", "tid", "t", "coef", "rewards")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _unet(cuda, r, alpha=None, cfg=None, b_std=0.05):
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = cfg or UNetConfig.tiny(16)
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r if alpha is None else alpha))
    unet.lora.init_gaussian(seed=1, b_std=b_std)
    unet.prepare()
    return unet


def _inputs(cuda, cfg, B=2, seed=0):
    """NCHW fp32 sample (element-type valued), timesteps, text states, pooled text, time ids."""
    g = _gen(seed)
    h = cfg.sample_size
    sample = torch.randn(B, 4, h, h, device=cuda, generator=g).to(ELEM).float()
    t = torch.tensor([999.0, 499.0][:B], device=cuda)
    enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(ELEM)
    text = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).to(ELEM)
    S = 8 * h
    tid = torch.tensor([[S, S, 0, 0, S, S]] * B, device=cuda, dtype=torch.float32)
    return sample, t, enc, text, tid


def _nhwc(sample):
    from pairwise_sample_optimization_amd import kernels as K
    return K.nchw_to_nhwc(sample)


def _fwd_bwd(unet, inp, dout=None, zero=True):
    """One forward_nhwc / backward_nhwc pass; returns (eps, the flat logical gradient afterwards)."""
    sample, t, enc, text, tid = inp
    eps, rt = unet.forward_nhwc(_nhwc(sample), t, enc, text, tid, save=True)
    if dout is None:
        dout = torch.randn(eps.shape, device=eps.device, generator=_gen(5)).to(ELEM)
    if zero:
        unet.lora.grad.zero_()
    unet.backward_nhwc(dout, rt)
    torch.cuda.synchronize()
    return eps, unet.lora.grad.clone()


# ----------------------------------------------------------------------------------------------------------------------
# 1. pack, bit-exact
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,alpha", [(3, 3), (4, 4), (4, 3)])
def test_pack_is_the_cast_and_scale_with_zero_pads(cuda, r, alpha):
    """Every padded working copy: logical part == ELEM(master) for A, ELEM(scale * ELEM(master)) for B (torch's
    arithmetic: the cast, then the product rounded in the element type), pads exactly zero; the transposed copies and
    the k/v stacks are built from them.  alpha 3 at r 4: scale 0.75, the pre-scale branch."""
    unet = _unet(cuda, r, alpha)
    st = unet.lora
    assert (st.r, st.r_pad, st.scale) == (r, 8, alpha / r)
    assert st.work.dtype == ELEM and st.work.numel() == st.master.numel() // r * 8
    torch.cuda.synchronize()
    covered = 0
    for name in st.adapter_names():
        A, B = st.adapter_views(st.master, name)
        Ap, Bp = st.adapter_views(st.work, name, padded=True)
        assert tuple(Ap.shape) == (8, A.shape[1]) and tuple(Bp.shape) == (B.shape[0], 8)
        assert torch.equal(Ap[:r], A.to(ELEM)), name
        assert torch.equal(Bp[:, :r], (st.scale * B.to(ELEM)).to(ELEM)), name
        assert Bp[:, :r].abs().max() > 0
        assert (Ap[r:].view(torch.int16) == 0).all() and (Bp[:, r:].view(torch.int16) == 0).all(), name
        covered += Ap.numel() + Bp.numel()
    assert covered == st.work.numel()  # the adapters tile the padded buffer: no element left unchecked
    for L in st.blk.values():
        for src, dst in ((L.A_qkv, L.At_qkv), (L.sB_qkv, L.sBt_qkv), (L.A_o1, L.At_o1), (L.sB_o1, L.sBt_o1),
                         (L.A_q2, L.At_q2), (L.sB_q2, L.sBt_q2), (L.sB_kv2, L.sBt_kv2), (L.A_o2, L.At_o2),
                         (L.sB_o2, L.sBt_o2)):
            assert torch.equal(dst, src.t())
    for A, sB, bl in st.kv_stacks.values():
        assert torch.equal(A, torch.cat([L.A_kv2 for L in bl], 0))
        assert torch.equal(sB, torch.cat([L.sB_kv2 for L in bl], 0))
    # a second pack after the master changed rewrites everything (and is what refresh(cast=False) runs too)
    st.master.mul_(-2.0)
    st.refresh(cast=False)
    A, _ = st.adapter_views(st.master, next(iter(st.adapter_names())))
    Ap, _ = st.adapter_views(st.work, next(iter(st.adapter_names())), padded=True)
    assert torch.equal(Ap[:r], A.to(ELEM)) and (Ap[r:].view(torch.int16) == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. equals the zero-padded wide adapter
# ----------------------------------------------------------------------------------------------------------------------
def _wide_twin(cuda, narrow):
    """An r_pad adapter whose A rows / B columns below r are the narrow one's, the rest zero, at the same scale."""
    n = narrow.lora
    wide = _unet(cuda, n.r_pad, n.alpha * n.r_pad / n.r)
    w = wide.lora
    assert w.scale == n.scale and w.grad_pad is None
    for name in n.adapter_names():
        (An, Bn), (Aw, Bw) = n.adapter_views(n.master, name), w.adapter_views(w.master, name)
        Aw.zero_()
        Bw.zero_()
        Aw[:n.r].copy_(An)
        Bw[:, :n.r].copy_(Bn)
    w.refresh()
    return wide


@pytest.mark.parametrize("r,alpha", [(4, 4), (4, 3), (3, 3)])
def test_equals_the_zero_padded_rank8_adapter(cuda, r, alpha):
    """Forward eps bit-identical to the rank-8 adapter with zero pads; after one backward from zeroed gradients the
    logical gradients equal that adapter's logical part -- bit for bit when the wide run is itself bit-reproducible
    (measured here), else within 4 x its run-to-run distance -- and the wide adapter's pad gradients are exactly 0."""
    from pairwise_sample_optimization_amd.unet import UNetConfig
    narrow = _unet(cuda, r, alpha)
    wide = _wide_twin(cuda, narrow)
    n, w = narrow.lora, wide.lora
    assert torch.equal(n.work, w.work)  # the padded working copy IS the wide adapter's
    inp = _inputs(cuda, UNetConfig.tiny(16))
    eps_n, g_n = _fwd_bwd(narrow, inp)
    eps_w, g_w1 = _fwd_bwd(wide, inp)
    _, g_w2 = _fwd_bwd(wide, inp)
    assert torch.equal(eps_n, eps_w)
    assert torch.isfinite(g_n).all() and g_n.abs().max() > 0
    noise = (g_w1 - g_w2).norm().item()
    dist = 0.0
    for name in n.adapter_names():
        for lo, wd, is_b in zip(n.adapter_views(g_n, name), w.adapter_views(g_w1, name), (False, True)):
            part, pad = (wd[:, :r], wd[:, r:]) if is_b else (wd[:r], wd[r:])
            assert (pad == 0).all(), name
            dist += (lo - part).double().pow(2).sum().item()
            if noise == 0.0:
                assert torch.equal(lo, part), name
    dist = dist ** 0.5
    print(f"r={r} alpha={alpha}: wide run-to-run |dg| = {noise:.3e}, narrow vs wide logical part |dg| = {dist:.3e}")
    assert dist <= 4.0 * noise
    assert (n.grad_pad == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3. parity against the fp32 oracle (the bars of tests/test_gpu_unet.py)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,r", [("tiny16", 1), ("tiny16", 3), ("tiny16", 4), ("tiny16", 7), ("sdxl32", 4)])
def test_forward_and_lora_grad_parity_vs_fp32_oracle(cuda, which, r):
    from oracle import sdxl_ref
    from pairwise_sample_optimization_amd.unet import UNetConfig
    cfg = UNetConfig.tiny(16) if which == "tiny16" else UNetConfig.sdxl(32)
    unet = _unet(cuda, r, cfg=cfg)
    st = unet.lora
    sample, t, enc, text, tid = _inputs(cuda, cfg)
    G = torch.randn(sample.shape, device=cuda, generator=_gen(5))
    st.grad.zero_()
    out = unet(sample, t, enc, added_cond_kwargs={"text_embeds": text, "time_ids": tid}).sample
    (out * G).sum().backward()
    torch.cuda.synchronize()
    mine = {k: v.clone() for k, v in st.grad_dict_peft().items()}
    leaf = {k: v.float().clone().requires_grad_(True) for k, v in st.state_dict_peft().items()}
    assert all(v.shape[0] == r for k, v in leaf.items() if "lora_A" in k)
    assert all(v.shape[1] == r for k, v in leaf.items() if "lora_B" in k)
    sd = sdxl_ref.sd_to(unet.state_dict(), cuda)
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)
    ref = sdxl_ref.unet_forward(sd, sample, t, enc.float(), text.float(), tid, lora=leaf, cfg=ocfg)
    (ref * G).sum().backward()
    e = _rel(out.detach(), ref.detach())
    num = sum((mine[k] - v.grad).norm().item() ** 2 for k, v in leaf.items())
    den = sum(v.grad.norm().item() ** 2 for v in leaf.values())
    tot = (num / den) ** 0.5
    print(f"{which} r={r}: eps rel err {e:.3e} (bar 3e-2), lora grad rel err total {tot:.3e} (bar 5e-2)")
    assert e < 3e-2
    assert den > 0 and tot < 5e-2
    assert (st.grad_pad == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4. fold semantics
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 4])
def test_fold_adds_once_and_clears_the_scratch(cuda, r):
    """grad_pad is all zero after a backward; zeroing lora.grad and running again gives a fresh state's bits; two
    backwards without zeroing give torch's fp32 g1 + g2 of the two single-backward gradients (one add per fold)."""
    from pairwise_sample_optimization_amd.unet import UNetConfig
    cfg = UNetConfig.tiny(16)
    unet = _unet(cuda, r)
    st = unet.lora
    inp = _inputs(cuda, cfg)
    d1 = torch.randn(2, 16, 16, 4, device=cuda, generator=_gen(5)).to(ELEM)
    d2 = torch.randn(2, 16, 16, 4, device=cuda, generator=_gen(6)).to(ELEM)
    _, g1 = _fwd_bwd(unet, inp, d1)
    assert (st.grad_pad.view(torch.int32) == 0).all()
    _, g2 = _fwd_bwd(unet, inp, d2)
    assert (st.grad_pad.view(torch.int32) == 0).all()
    _, g1_again = _fwd_bwd(unet, inp, d1)  # after lora.grad.zero_(), on a state that has run other backwards
    fresh = _unet(cuda, r)
    _, g1_fresh = _fwd_bwd(fresh, inp, d1)
    assert g1.abs().max() > 0 and not torch.equal(g1, g2)
    assert torch.equal(g1_again, g1) and torch.equal(g1_fresh, g1)
    _fwd_bwd(unet, inp, d1)
    _, g12 = _fwd_bwd(unet, inp, d2, zero=False)
    assert torch.equal(g12, g1 + g2)
    assert (st.grad_pad.view(torch.int32) == 0).all()
    # a caller-side K.zero_ of the gradient (lora_optimizer_step's) leaves nothing behind in the scratch either
    from pairwise_sample_optimization_amd import kernels as K
    K.zero_(st.grad)
    _, g2_again = _fwd_bwd(unet, inp, d2, zero=False)
    assert torch.equal(g2_again, g2)


# ----------------------------------------------------------------------------------------------------------------------
# trainer fixtures
# ----------------------------------------------------------------------------------------------------------------------
def _trainer(cuda, r=4, use_8bit_adam=False, lr=1e-3, seed=None, **kw):
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    unet.lora.init_gaussian(seed=1 if seed is None else seed, b_std=0.05)
    unet.prepare()
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, gradient_accumulation_steps=1, train_batch_size=1, lr=lr,
                    use_8bit_adam=use_8bit_adam, loss_scale=256.0 if F16 else None, **kw)
    return unet, tr


@pytest.fixture(scope="module")
def stream4(cuda):
    """One shuffled sample buffer of the tiny r = 4 trainer (one accumulation window), shared and left unchanged."""
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNetConfig
    cfg = UNetConfig.tiny(16)
    _, tr = _trainer(cuda)
    g = _gen(3)
    enc = torch.randn(1, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(ELEM)
    pooled = torch.randn(1, cfg.text_embed_dim, device=cuda, generator=g).to(ELEM)
    tid = compute_time_ids(128, 0, cuda)
    buf = tr.sample_pairs(enc, pooled, tid, 16, generator=g,
                          reward_fn=lambda x: torch.rand(x.shape[0], device=cuda, generator=g))
    return tr.shuffle(buf, generator=_gen(100))


# ----------------------------------------------------------------------------------------------------------------------
# 5. side stream and hipGraph
# ----------------------------------------------------------------------------------------------------------------------
def test_backward_side_stream_equals_in_line(cuda, stream4):
    """The weight-gradient products AND the fold on the side stream (PSO_SIDE_STREAM path) give the in-line bits: the
    fold is ordered after its unit's products, and the final join leaves the gradient complete, the scratch zero."""
    from pairwise_sample_optimization_amd import kernels as K
    unet, tr = _trainer(cuda)
    tr.auto_step = False
    grads = []
    for side in (False, True, False):
        K.SideStream.enabled = side
        try:
            unet.lora.grad.zero_()
            tr.micro_step(tr.micro_batch(stream4, 0, 1))
            torch.cuda.synchronize()
            grads.append(unet.lora.grad.clone())
            assert (unet.lora.grad_pad == 0).all()
        finally:
            K.SideStream.enabled = False
    assert grads[0].abs().max() > 0 and torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[2])
    assert torch.equal(grads[0], grads[1])


def test_graph_epoch_gradient_equals_eager_epoch(cuda, stream4):
    """train_epoch_graph (pack, products and folds replayed from a hipGraph) == train_epoch, gradient bits and the
    masters after the step before it."""
    u_g, tr_g = _trainer(cuda)
    u_e, tr_e = _trainer(cuda)
    tr_g.train_epoch_graph(stream4)
    tr_e.train_epoch(stream4)
    assert tr_g._graph is not None and tr_g.opt_step == tr_e.opt_step == 1
    assert torch.equal(u_g.lora.master, u_e.lora.master) and torch.equal(u_g.lora.work, u_e.lora.work)
    seen = {}
    for name, tr, u in (("graph", tr_g, u_g), ("eager", tr_e, u_e)):
        tr.optimizer_step = lambda u=u, name=name: seen.__setitem__(name, u.lora.grad.clone())
    tr_g.train_epoch_graph(stream4)
    tr_e.train_epoch(stream4)
    torch.cuda.synchronize()
    assert seen["eager"].abs().max().item() > 0 and torch.isfinite(seen["eager"]).all()
    assert torch.equal(seen["graph"], seen["eager"])
    assert (u_g.lora.grad_pad == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 6. optimizer step on peft's tensors
# ----------------------------------------------------------------------------------------------------------------------
def test_adamw_step_vs_float64_on_peft_tensors(cuda, stream4):
    """One fp32 AdamW step: every peft-shaped tensor of the master equals float64 AdamW applied to the HIP gradient of
    that tensor (the kernel's own clip coefficient, the loss scale undone), within 1e-6 max|ref| -- the bar of
    tests/test_gpu_optim.py::test_adamw_step_vs_float64."""
    F32 = np.float32
    lr, b1, b2, eps, wd = (float(F32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 1e-6))
    unet, tr = _trainer(cuda, lr=1e-3)
    st = unet.lora
    tr.auto_step = False
    tr.train_epoch(stream4)
    torch.cuda.synchronize()
    p0 = {k: v.double().cpu().numpy() for k, v in st.state_dict_peft().items()}
    g = {k: v.double().cpu().numpy() for k, v in st.grad_dict_peft().items()}
    assert all(v.shape[0] == 4 for k, v in p0.items() if "lora_A" in k)
    tr.optimizer_step()
    torch.cuda.synchronize()
    s = float(tr.clip_buf[1].item()) / tr.loss_scale
    p1 = {k: v.double().cpu().numpy() for k, v in st.state_dict_peft().items()}
    worst, moved = 0.0, 0.0
    for k in p0:
        gi = g[k] * s
        m = (1.0 - b1) * gi
        v = (1.0 - b2) * gi * gi
        ref = p0[k] * (1.0 - lr * wd) - lr / (1.0 - b1) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2) + eps))
        worst = max(worst, np.abs(p1[k] - ref).max() / np.abs(ref).max())
        moved = max(moved, np.abs(ref - p0[k]).max())
    print(f"r=4 AdamW step vs float64 on {len(p0)} peft tensors: worst max|diff| / max|ref| = {worst:.2e}")
    assert moved > 1e-4 and tr.opt_step == 1
    assert worst <= 1e-6
    assert (st.grad == 0).all()
    w = st.work.clone()
    st.refresh()
    assert torch.equal(w, st.work)


def test_adamw8bit_step_keeps_32bit_state_and_repacks(cuda, stream4):
    """use_8bit_adam at r = 4 on the tiny UNet: every peft tensor is below 4096 elements, so the whole state is 32-bit
    (padded to rank 8 the 8 x 128 A tensors would still be, but SDXL's 4 x 640 ones would not); the step runs, and
    the padded working copies after it are a fresh pack of the new master (the fused 16-bit write is not used)."""
    from pairwise_sample_optimization_amd.trainer import _work_copy, trainable_segments
    unet, tr = _trainer(cuda, use_8bit_adam=True)
    st = unet.lora
    segs = trainable_segments(unet)
    assert max(n for _, n in segs) < tr.adam8.MIN_8BIT_SIZE and sum(n for _, n in segs) == st.master.numel()
    assert all(row[2] >= 0 for row in tr.adam8.rows)  # every block has a 32-bit slot
    assert _work_copy(unet, st.master) is None
    m0 = st.master.clone()
    tr.train_epoch(stream4)
    torch.cuda.synchronize()
    assert tr.opt_step == 1 and torch.isfinite(st.master).all() and not torch.equal(st.master, m0)
    assert tr.adam8.m32.abs().max() > 0 and tr.adam8.v32.abs().max() > 0
    assert (tr.adam8.qm == 0).all() and (tr.adam8.qv == 0).all()  # no 8-bit codes written
    assert (st.grad == 0).all() and (st.grad_pad == 0).all()
    w = st.work.clone()
    for name in st.adapter_names():
        A, _ = st.adapter_views(st.master, name)
        Ap, _ = st.adapter_views(w, name, padded=True)
        assert torch.equal(Ap[:4], A.to(ELEM)) and (Ap[4:] == 0).all()
    st.refresh()
    assert torch.equal(w, st.work)


# ----------------------------------------------------------------------------------------------------------------------
# 7. overlapped gradient sync (world 1, RCCL, in a child process as tests/test_gpu_dist.py runs its ranks)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_overlapped_sync_equals_flat_sync_world1(cuda, tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, os.path.join(HERE, "lora_narrow_rank_worker_gpu.py"), "--out", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(os.path.join(tmp_path, "rank0.json")))
    print(d)
    assert d["backend"] == "nccl" and d["world"] == 1 and d["rank"] == 4
    assert d["buckets"] >= 3 and d["issued_before_finish"] == d["buckets"]
    assert d["grad_norm"] > 0
    assert d["bucketed_equals_flat"] and d["masters_equal"] and d["scratch_zero"]


# ----------------------------------------------------------------------------------------------------------------------
# 8. checkpoints
# ----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_is_bit_exact_and_holds_peft_shapes(cuda, stream4, tmp_path):
    from safetensors.torch import load_file
    from pairwise_sample_optimization_amd import lora_io
    u_a, tr_a = _trainer(cuda)
    tr_a.train_epoch(stream4)
    tr_a.train_epoch(stream4)
    u_b, tr_b = _trainer(cuda)
    tr_b.train_epoch(stream4)
    lora_io.save_state(tr_b, str(tmp_path))
    u_c, tr_c = _trainer(cuda, seed=9)  # other initial adapters: everything must come from the checkpoint
    assert not torch.equal(u_c.lora.master, u_b.lora.master)
    lora_io.load_state(tr_c, str(tmp_path))
    assert torch.equal(u_c.lora.master, u_b.lora.master) and torch.equal(u_c.lora.work, u_b.lora.work)
    assert (tr_c.opt_step, tr_c.n_micro) == (1, 1)
    tr_c.train_epoch(stream4)
    torch.cuda.synchronize()
    assert tr_a.opt_step == tr_c.opt_step == 2
    assert torch.equal(u_c.lora.master, u_a.lora.master)
    assert torch.equal(tr_c.exp_avg, tr_a.exp_avg) and torch.equal(tr_c.exp_avg_sq, tr_a.exp_avg_sq)
    sd = load_file(os.path.join(tmp_path, lora_io.LORA_WEIGHT_NAME))
    names = list(u_b.lora.adapter_names())
    assert len(sd) == 2 * len(names)
    for name in names:
        down, up = sd[f"unet.{name}.lora.down.weight"], sd[f"unet.{name}.lora.up.weight"]
        assert down.shape[0] == 4 and up.shape[1] == 4 and down.shape[1] == 128 and up.shape[0] == 128
    opt = load_file(os.path.join(tmp_path, lora_io.OPT_NAME))
    assert opt["exp_avg"].numel() == u_b.lora.master.numel()
    # the rank-4 file does not fit a rank-8 adapter: a ValueError naming both ranks, not a copy_ shape error
    u8 = _unet(cuda, 8)
    with pytest.raises(ValueError, match=r"rank 4 .*rank 8"):
        lora_io.load_lora_into_unet(sd, None, u8)


# ----------------------------------------------------------------------------------------------------------------------
# 9. DreamBooth (the reference script's default --rank=4)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(F16, reason="DreamBoothPSOTrainer raises under the f16 library by design (no loss scaler)")
def test_dreambooth_micro_step_rank4_vs_fp32_reference(cuda):
    """The pso_db, B = 1 case of tests/test_gpu_dreambooth.py at r = 4, its bars: loss rel < 2e-2, grad rel < 1e-1."""
    from oracle import sdxl_ref
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.dreambooth import DreamBoothPSOTrainer
    from pairwise_sample_optimization_amd.trainer import compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    from pairwise_sample_optimization_amd.vae import AutoencoderKL, VAEConfig
    cfg = UNetConfig.tiny(16)
    B, beta = 1, 5.0
    with torch.device(cuda):
        unet = UNet2DConditionModel(cfg)
        vae = AutoencoderKL(VAEConfig.tiny())
    unet.init_weights(0)
    vae.init_weights(2)
    unet.add_adapter(SimpleNamespace(r=4, lora_alpha=4))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    tr = DreamBoothPSOTrainer(unet, vae, loss_type="pso_db", beta_pso=beta, gradient_accumulation_steps=1)
    tr.auto_step = False
    assert tr.exp_avg.numel() == unet.lora.master.numel()
    g = _gen(4)
    pix = torch.rand(2 * B, 3, 128, 128, device=cuda, generator=g) * 2 - 1
    enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).bfloat16()
    pooled = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).bfloat16()
    tid = compute_time_ids(128, 0, cuda).repeat(B, 1)
    st = unet.lora
    st.grad.zero_()
    loss = tr.micro_step(pix, enc, pooled, tid, generator=_gen(11)).item()
    mine = {k: v.clone() for k, v in st.grad_dict_peft().items()}
    inp = tr.prepare_inputs(pix, _gen(11))
    sd = sdxl_ref.sd_to(unet.state_dict(), cuda)
    leaf = {k: v.float().clone().requires_grad_(True) for k, v in st.state_dict_peft().items()}
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)
    x_in = K.nhwc_to_nchw(inp["unet_in"]).float()
    e2, p2, t2 = enc.float().repeat(2, 1, 1), pooled.float().repeat(2, 1), tid.repeat(2, 1)
    ep = sdxl_ref.unet_forward(sd, x_in, inp["t"], e2, p2, t2, lora=leaf, cfg=ocfg)
    ep = ep + (ep.bfloat16().float() - ep).detach()  # bf16-autocast output values, fp32 gradient path
    s = inp["sigma"].view(-1, 1, 1, 1)
    nz, x0 = inp["noisy"].permute(0, 3, 1, 2), inp["x0"].permute(0, 3, 1, 2)
    per = lambda e: ((s ** -2.0) * ((e * (-s) + nz) - x0) ** 2).reshape(2 * B, -1).mean(1)
    lw, ll = per(ep).chunk(2)
    ref = torch.relu(1 - beta * (-(lw - 0.1 * ll))).mean() + 0.5 * ll.mean()
    ref.backward()
    rel = abs(loss - ref.item()) / abs(ref.item())
    num = sum(((mine[k] - v.grad) ** 2).sum().item() for k, v in leaf.items())
    den = sum((v.grad ** 2).sum().item() for v in leaf.values())
    grel = (num / max(den, 1e-30)) ** 0.5
    print(f"pso_db B=1 r=4: loss mine={loss:.6f} fp32-ref={ref.item():.6f} rel={rel:.2e} grad rel={grel:.3e}")
    assert rel < 2e-2
    assert den > 0 and grel < 1e-1
    # and the optimizer step of the trainer (fp32 AdamW on the logical tensors) runs and repacks
    tr.optimizer_step()
    torch.cuda.synchronize()
    assert tr.opt_step == 1 and torch.isfinite(st.master).all() and (st.grad == 0).all() and (st.grad_pad == 0).all()
