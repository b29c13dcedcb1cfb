"""Child process of tests/test_gpu_clip_f16.py (PSO_LIB=f16: the element type is per process): the CLIP towers, the
PickScore reward and one whole online PSO epoch (sample -> VAE decode -> PickScore reward -> train) on the fp16
library, opted in with allow_f16=True.

Cases, in order; the process ends at the first failure (a GPU fault ends it there too):
  a. the default refusals still stand (the three calls tests/test_gpu_f16.py pins)
  b. attention_small on fp16 inputs against fp32 torch softmax attention
  c. pso_clip_preprocess_img: fp16 images bit-exact against torch fp16 quantisation + PIL; f32 / uint8 images equal
     the bits of pso_clip_preprocess
  d. two small text towers against transformers fp32, yardstick: the same transformers module in .half()
  e. PickScore at real width and reduced depth against transformers fp32 / .half()
  f. one epoch in one process: encode_prompt -> PSOTrainer.sample_pairs(reward_fn=pickscore_reward,
     decode_fn=vae.decode_latents_nhwc) -> shuffle -> train_epoch

`--figures` prints the error figures of (d) and (e) and asserts nothing: run under the bf16 library it gives that
library's errors at the same shapes."""
import copy
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUDA = torch.device("cuda:0")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ids(B, S, vocab, g):
    """tests/test_gpu_clip.py::_ids: bos, tokens, eos (the max id: the legacy argmax pooling row), eos padding."""
    ids = torch.randint(1, vocab - 2, (B, S), generator=g, device=CUDA)
    ids[:, 0] = vocab - 2
    for b in range(B):
        n = 5 + 17 * b
        ids[b, n] = vocab - 1
        ids[b, n + 1:] = vocab - 1
    return ids


def _tensor(x, *names):
    """transformers 4.x returns a tensor from get_*_features, 5.x an output object."""
    if torch.is_tensor(x):
        return x
    for n in names:
        if getattr(x, n, None) is not None:
            return getattr(x, n)
    raise TypeError(type(x))


class Yardstick:
    """tests/test_gpu_f16.py::_yardstick: finite, and rel(ours, fp32) <= 1.5 x rel(torch fp16, fp32)."""

    def __init__(self, check):
        self.check = check

    def __call__(self, name, mine, torch16, ref32):
        e, y = _rel(mine, ref32), _rel(torch16, ref32)
        print(f"  {name}: library {e:.3e}  torch fp16 {y:.3e}  (bar 1.5x = {1.5 * y:.3e})", flush=True)
        if self.check:
            assert torch.isfinite(mine.float()).all(), name
            assert e <= 1.5 * y, (name, e, y)


# ----------------------------------------------------------------------------------------------------------------------
def case_a_refusals():
    import pytest
    from pairwise_sample_optimization_amd import _lib, clip
    from pairwise_sample_optimization_amd import kernels as K
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        clip.CLIPTextModel(clip.CLIPTextConfig())
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        clip.CLIPVisionTransformer(clip.CLIPVisionConfig())
    with pytest.raises(_lib.PsoLibError, match="f16 library"):
        K.clip_preprocess(torch.zeros(1, 32, 32, 3, device=CUDA, dtype=torch.float16), 28, 14, 592, (0.5,) * 3,
                          (0.5,) * 3)
    print("a. refusals intact", flush=True)


def case_b_attention():
    """Everything before the output's rounding is fp32, so the error is that rounding: at most 2^-11 (4.9e-4) per
    element.  The bar is twice that."""
    from pairwise_sample_optimization_amd import kernels as K
    B = 2
    for S, D, H, causal in ((77, 64, 2, True), (257, 80, 2, False), (50, 80, 2, True), (130, 128, 1, False)):
        qkv = torch.randn(B * S, 3 * H * D, device=CUDA, generator=_gen(S + D)).half()
        C = H * D
        o = K.attention_small(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, S, H, causal, D ** -0.5)
        f = lambda t: t.float().reshape(B, S, H, D).transpose(1, 2)
        q, k, v = f(qkv[:, :C]), f(qkv[:, C:2 * C]), f(qkv[:, 2 * C:])
        s = q @ k.transpose(-1, -2) * D ** -0.5
        if causal:
            s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=CUDA), 1), float("-inf"))
        ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * S, C)
        e = _rel(o, ref)
        print(f"b. attention_small S={S} D={D} H={H} causal={causal}: rel L2 {e:.3e} (bar 1e-3)", flush=True)
        assert o.dtype == torch.float16 and torch.isfinite(o).all()
        assert e < 1e-3, (S, D, H, causal, e)


def _image(B, H, W, seed):
    """tests/test_gpu_clip.py::test_clip_preprocess_bit_exact_vs_pil: smooth structure + noise, with values outside
    [-1, 1] (clamped by the quantisation); fp32."""
    g = _gen(seed)
    yy, xx = torch.linspace(-1.2, 1.2, H, device=CUDA), torch.linspace(-1.2, 1.2, W, device=CUDA)
    return (yy[None, :, None, None] * xx[None, None, :, None] * torch.randn(B, 1, 1, 3, device=CUDA, generator=g)
            + 0.3 * torch.randn(B, H, W, 3, device=CUDA, generator=g)).contiguous()


def case_c_preprocess():
    """One uint8 step moves a normalised value by >= 1 / (255 * 0.276) = 0.014; the fp16 ulp below 4 is 0.002: equality
    pins every resized byte.  The reference quantises the fp16 CPU tensor as torch executes the trainer's line."""
    from oracle.clip_ref import clip_image_processor, trainer_uint8
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.clip import CLIP_MEAN, CLIP_STD
    l = _lib.lib()
    m, sd = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
    for B, H, W, size in ((2, 96, 72, 28), (1, 64, 64, 28), (1, 40, 56, 56)):
        img32 = _image(B, H, W, H + W)
        img = img32.half().contiguous()
        assert (img.abs() > 1).any()
        patches = K.clip_preprocess(img, size, 14, 592, CLIP_MEAN, CLIP_STD, allow_f16=True)
        u8 = trainer_uint8(img.permute(0, 3, 1, 2).cpu())
        u8_f32 = trainer_uint8(img.float().permute(0, 3, 1, 2).cpu())
        ref = K.patchify(torch.from_numpy(clip_image_processor(u8, size=size)).to(CUDA), 14, 592)
        print(f"c. preprocess fp16 B={B} {H}x{W} -> {size}: {(u8 != u8_f32).mean() * 100:.1f} % of the bytes differ "
              f"from fp32 quantisation; patches differing from the reference: {(patches != ref).sum().item()}",
              flush=True)
        assert patches.dtype == torch.float16 and tuple(patches.shape) == (B * (size // 14) ** 2, 592)
        assert torch.equal(patches, ref), (patches.float() - ref.float()).abs().max().item()
        # f32 and uint8 images: the bits of the old entry, called directly (kernels.clip_preprocess refuses under f16)
        for x, code in ((img32, _lib.PSO_F32), (torch.from_numpy(np.ascontiguousarray(u8)).to(CUDA), 2)):  # PSO_U8
            new = K.clip_preprocess(x, size, 14, 592, CLIP_MEAN, CLIP_STD, allow_f16=True)
            ws = torch.empty(l.pso_clip_preprocess_ws_bytes(B, H, W, size), device=CUDA, dtype=torch.uint8)
            old = torch.full_like(new, float("nan"))
            _lib.check(l.pso_clip_preprocess(B, H, W, x.data_ptr(), code, size, 14, 592, m, sd, old.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "pso_clip_preprocess")
            assert torch.equal(new, old), (str(x.dtype), H, W)
        assert torch.equal(K.clip_preprocess(torch.from_numpy(np.ascontiguousarray(u8)).to(CUDA), size, 14, 592,
                                             CLIP_MEAN, CLIP_STD, allow_f16=True), ref)


def case_d_text(yard):
    from oracle.clip_ref import hf_text_model
    from pairwise_sample_optimization_amd.clip import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    for hidden, act, cls in ((128, "quick_gelu", CLIPTextModel), (160, "gelu", CLIPTextModelWithProjection)):
        cfg = CLIPTextConfig(vocab_size=1000, hidden_size=hidden, intermediate_size=4 * hidden, num_hidden_layers=2,
                             num_attention_heads=2, hidden_act=act, projection_dim=hidden)
        with torch.device(CUDA):
            m = cls(cfg, allow_f16=True)
        m.init_weights(3)
        hf = hf_text_model(cfg, m.state_dict(), CUDA, projection=cls is CLIPTextModelWithProjection)
        hf16 = copy.deepcopy(hf).half()
        ids = _ids(3, 77, cfg.vocab_size, _gen(5))
        out = m(ids, output_hidden_states=True)
        with torch.no_grad():
            ref, t16 = hf(ids, output_hidden_states=True), hf16(ids, output_hidden_states=True)
        print(f"d. text tower hidden {hidden} ({act}, {cls.__name__})", flush=True)
        yard("hidden_states[-2]", out.hidden_states[-2], t16.hidden_states[-2], ref.hidden_states[-2])
        yard("last_hidden_state", out.last_hidden_state, t16.last_hidden_state, ref.last_hidden_state)
        yard("out[0]", out[0], t16[0], ref[0])


def case_e_pickscore(yard):
    from oracle.clip_ref import clip_image_processor, hf_clip_model, trainer_uint8
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.clip import CLIPTextConfig, CLIPVisionConfig
    from pairwise_sample_optimization_amd.pso_pytorch.pickscore_utils import Selector
    tc = CLIPTextConfig(vocab_size=1000, hidden_size=1024, intermediate_size=4096, num_hidden_layers=2,
                        num_attention_heads=16, hidden_act="gelu", projection_dim=1024)
    vc = CLIPVisionConfig(num_hidden_layers=4)  # 1280 wide, 16 heads, 5120 intermediate, 224 / 14, projection 1024
    sel = Selector(CUDA, seed=4, text_config=tc, vision_config=vc, allow_f16=True)
    m = sel.model
    hf = hf_clip_model(m.text_config, m.vision_config, m.config.projection_dim, m.state_dict(), CUDA)
    hf16 = copy.deepcopy(hf).half()
    g = _gen(13)
    B = 2
    img = (0.6 * torch.randn(B, 256, 256, 3, device=CUDA, generator=g)).clamp(-1, 1).to(_lib.ELEM_DTYPE).contiguous()
    ids = _ids(B, 77, tc.vocab_size, g)
    s = sel.score_tensor(img, ids)
    u8 = trainer_uint8(img.permute(0, 3, 1, 2).cpu())
    pv = torch.from_numpy(clip_image_processor(u8)).to(CUDA)
    with torch.no_grad():
        ie = _tensor(hf.get_image_features(pixel_values=pv), "image_embeds", "pooler_output")
        te = _tensor(hf.get_text_features(input_ids=ids), "text_embeds", "pooler_output")
        ie16 = _tensor(hf16.get_image_features(pixel_values=pv.half()), "image_embeds", "pooler_output")
        te16 = _tensor(hf16.get_text_features(input_ids=ids), "text_embeds", "pooler_output")
        ref = torch.nn.functional.cosine_similarity(te, ie, dim=-1)
        ref16 = torch.nn.functional.cosine_similarity(te16.float(), ie16.float(), dim=-1)
        ours_ie = m.image_features_from_images(img)
        ours_te = m.get_text_features(ids)
    print("e. PickScore at real width (vision 1280 x 4 layers, text 1024 x 2 layers), 2 images of 256^2", flush=True)
    yard("image features", ours_ie, ie16, ie)
    yard("text features", ours_te, te16, te)
    d, d16 = (s - ref).abs().max().item(), (ref16 - ref).abs().max().item()
    print(f"  score: ours {s.tolist()} fp32 {ref.tolist()}: max |diff| library {d:.3e}  torch fp16 {d16:.3e} "
          "(bar 2e-3)", flush=True)
    s2 = sel.score(list(u8), None, input_ids=ids)
    d2 = float(np.abs(s2 - s.cpu().numpy()).max())
    print(f"  score(uint8 images) against score_tensor: {d2:.3e} (bar 1e-6)", flush=True)
    if yard.check:
        assert torch.isfinite(s).all() and d < 2e-3, (d, s.tolist(), ref.tolist())
        assert d2 < 1e-6, d2


def case_f_epoch():
    from pairwise_sample_optimization_amd.amp import DeviceLossScaler
    from pairwise_sample_optimization_amd.clip import CLIPTextConfig, CLIPVisionConfig
    from pairwise_sample_optimization_amd.prompts import encode_prompt, sdxl_text_encoders
    from pairwise_sample_optimization_amd.pso_pytorch.pickscore_utils import Selector
    from pairwise_sample_optimization_amd.rewards import pickscore_reward
    from pairwise_sample_optimization_amd.trainer import PSOTrainer, compute_time_ids
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    from pairwise_sample_optimization_amd.vae import AutoencoderKL, VAEConfig
    cfg = UNetConfig.tiny(16)
    with torch.device(CUDA):
        unet = UNet2DConditionModel(cfg)
        vae = AutoencoderKL(VAEConfig.tiny())
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    unet.prepare()
    vae.init_weights(0)
    vae.prepare()
    # prompt encoders: 64 + 64 = cross_attention_dim, projection 64 = text_embed_dim
    enc_cfg = lambda act: CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=256, num_hidden_layers=2,
                                         num_attention_heads=1, hidden_act=act, projection_dim=64)
    encoders = sdxl_text_encoders(CUDA, seed=1, configs=(enc_cfg("quick_gelu"), enc_cfg("gelu")), allow_f16=True)
    sel = Selector(CUDA, seed=2, allow_f16=True,
                   text_config=CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512,
                                              num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                                              projection_dim=64),
                   vision_config=CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2,
                                                  num_attention_heads=2, image_size=56, projection_dim=64))
    g = _gen(7)
    Bp = 2
    ids1, ids2, ids_r = (_ids(Bp, 77, 1000, g) for _ in range(3))
    enc, pooled = encode_prompt(encoders, [ids1, ids2])
    assert tuple(enc.shape) == (Bp, 77, cfg.cross_attention_dim) and tuple(pooled.shape) == (Bp, cfg.text_embed_dim)
    assert enc.dtype == pooled.dtype == torch.float16 and torch.isfinite(enc).all() and torch.isfinite(pooled).all()
    scaler = DeviceLossScaler(device=CUDA)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2, train_batch_size=1, loss_scale=scaler)
    reward_ids = ids_r.repeat_interleave(2, 0)  # image order 2b + k -> prompt b
    decoded = []

    def decode(x):
        decoded.append(vae.decode_latents_nhwc(x))
        return decoded[-1]

    buf = tr.sample_pairs(enc, pooled, compute_time_ids(128, 0, CUDA).repeat(Bp, 1), 16, generator=g,
                          reward_fn=pickscore_reward(sel, reward_ids), decode_fn=decode)
    rw = buf["rewards"]
    img = decoded[0]
    assert len(decoded) == 1 and img.dtype == torch.float16 and tuple(img.shape) == (2 * Bp, 128, 128, 3)
    assert tuple(rw.shape) == (Bp, 2, 1) and rw.dtype == torch.float32 and torch.isfinite(rw).all()
    again = sel.score_tensor(img, reward_ids).reshape(Bp, 2, 1)
    assert torch.equal(rw, again), (rw - again).abs().max().item()  # same kernels, same inputs: the same bits
    sb = tr.shuffle(buf, generator=_gen(100))
    windows = sb.n_micro // tr.gas_total
    step0, master0 = tr.opt_step, unet.lora.master.clone()
    tr.train_epoch(sb)
    torch.cuda.synchronize()
    losses = torch.stack([l.float().reshape(-1)[0] for l in tr.loss_hist])
    print(f"f. epoch: rewards {rw.flatten().tolist()} losses {losses.tolist()} opt_step {step0} -> {tr.opt_step} "
          f"({windows} windows, {scaler.skipped} skipped, scale {scaler.scale})", flush=True)
    assert len(tr.loss_hist) > 0 and torch.isfinite(losses).all()
    assert torch.isfinite(unet.lora.master).all() and not torch.equal(unet.lora.master, master0)
    assert windows == 2 and tr.opt_step - step0 == windows, (step0, tr.opt_step, windows, scaler.state_dict())


def main():
    from pairwise_sample_optimization_amd import _lib
    if "--figures" in sys.argv[1:]:
        print(f"figures only, element type {_lib.ELEM_DTYPE}", flush=True)
        yard = Yardstick(check=False)
        case_d_text(yard)
        case_e_pickscore(yard)
        print("CLIP_FIGURES_DONE", flush=True)
        return
    assert _lib.F16 and _lib.ELEM_DTYPE == torch.float16
    yard = Yardstick(check=True)
    case_a_refusals()
    case_b_attention()
    case_c_preprocess()
    case_d_text(yard)
    case_e_pickscore(yard)
    case_f_epoch()
    print("CLIP_F16_OK", flush=True)


if __name__ == "__main__":
    main()
