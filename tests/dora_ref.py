"""Restatement of peft 0.11's DoRA (DoraLinearLayer) for the tests, in plain torch and sharing no code with the product.

For an adapted Linear with base weight W [out, in], LoRA A [r, in], B [out, r], scaling s and magnitude m [out]:

    n = || W + s B A ||_2 per output row, DETACHED        (peft: weight_norm.detach())
    y = (m / n) . (x W^T + s x A^T B^T) + bias

`fold` writes that as a plain LoRA model with other weights -- W' = (m / n)[:, None] W and B' = s (m / n)[:, None] B --
so the unmodified oracle (oracle/sdxl_ref.unet_forward, whose LoRA scaling is 1) computes the DoRA forward, and torch
autograd through the fold gives peft's gradients for A, B and m: A and B reach the output through the LoRA term only
(n is detached), m through the column scale.  tests/test_dora_cpu.py checks the restatement against closed forms.

On the tiny16 UNet (CPU, fp32, B = 2, r = 8, A ~ N(0, 1) / r, B ~ 0.05 N(0, 1)) with m = n the folded model IS the
plain-LoRA one (rel 0.0), and with m = n 2^U(-1, 1) its eps and its A / B gradients move far from plain LoRA's; how far
depends on the draw of inputs, adapters and magnitudes, so each test prints its own figure and asserts only a ratio to
its parity bars (tests/test_dora_cpu.py::test_fold_moves_outputs_and_gradients, gpu_parity_case below).
"""
import torch

MAG = "lora_magnitude_vector"
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


def row_norms(W, A, B, scale):
    """||W + scale * B A|| per output row, detached."""
    return (W + scale * (B @ A)).norm(dim=1).detach()


def adapter_modules(lora):
    """Module paths that carry an adapter in a peft-named dict."""
    return sorted(k[:-len(".lora_A.weight")] for k in lora if k.endswith(".lora_A.weight"))


def norms(sd, lora, scale):
    """{module path: n} for every adapter of `lora` over the base weights `sd`."""
    return {p: row_norms(sd[p + ".weight"].detach(), lora[p + ".lora_A.weight"].detach(),
                         lora[p + ".lora_B.weight"].detach(), scale) for p in adapter_modules(lora)}


def fold(sd, lora, mags, scale):
    """(sd', lora') with W' = (m / n)[:, None] W and B' = scale (m / n)[:, None] B, n detached: the oracle's plain
    LoRA forward (scaling 1) on them is the DoRA forward.  mags = {module path: m [out]}; differentiable in A, B, m."""
    sd2, lora2 = dict(sd), dict(lora)
    for p in adapter_modules(lora):
        W, A, B = sd[p + ".weight"], lora[p + ".lora_A.weight"], lora[p + ".lora_B.weight"]
        g = mags[p] / row_norms(W.detach(), A.detach(), B.detach(), scale)
        sd2[p + ".weight"] = g[:, None] * W
        lora2[p + ".lora_B.weight"] = scale * g[:, None] * B
    return sd2, lora2


def dora_linear(x, W, A, B, m, scale, bias=None):
    """One DoRA Linear, written out (no fold): for the closed-form checks."""
    n = row_norms(W.detach(), A.detach(), B.detach(), scale)
    z = x @ W.t() + scale * (x @ A.t()) @ B.t()
    y = (m / n) * z
    return y if bias is None else y + bias


def spread(n, gen, width):
    """m = n * 2^U(-width, width): magnitudes away from the initial m = n, by up to a factor 2^width either way."""
    u = torch.rand(n.shape, generator=gen, device=n.device, dtype=n.dtype) * 2 - 1
    return n * torch.exp2(width * u)


def total_rel(got, ref, keys=None):
    """sqrt(sum |got - ref|^2 / sum |ref|^2) over the tensors named by keys (default: all of ref)."""
    keys = list(ref) if keys is None else list(keys)
    num = sum(((got[k].double() - ref[k].double()) ** 2).sum().item() for k in keys)
    den = sum((ref[k].double() ** 2).sum().item() for k in keys)
    return (num / den) ** 0.5


# ----------------------------------------------------------------------------------------------------------------------
# the UNet parity case on the GPU, shared by tests/test_gpu_dora.py and tests/dora_f16_worker_gpu.py
# ----------------------------------------------------------------------------------------------------------------------
FWD_BAR, GRAD_BAR = 3e-2, 5e-2  # tests/test_gpu_unet.py's bars for the same shapes
# magnitude spread m = n 2^U(-w, w) per shape.  The case must tell DoRA from plain LoRA by a wide margin (asserted
# from the oracle alone, gpu_parity_case: eps moved by >= 3 x 3e-2 = 0.09 rel).  With gpu_parity_case's own draws on
# an MI355X the oracle's eps moves by 0.19 (tiny16, r = 8), 0.22 (tiny16, r = 4) and 0.34 (sdxl32); tiny16 at w = 1
# lands near 0.1 -- too close to the 0.09 to rely on -- hence its wider spread.
WIDTHS = {"tiny16": 1.5, "sdxl32": 1.0}


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def gpu_parity_case(which, r, loss_scale=1.0):
    """The HIP UNet against the fp32 oracle on identical 16-bit-valued weights and inputs (B = 2), twice on the same
    UNet: with a plain LoRA adapter, then with a DoRA adapter of the same A / B (B != 0) and m = n 2^U(-w, w).
    loss_scale: factor on the loss of the HIP backward, divided out of its gradients (fp16 runs).  Returns a namespace
    of the UNet (DoRA adapter on), its inputs, and the errors; asserts nothing but that the two adapters share A, B."""
    from types import SimpleNamespace
    from oracle import sdxl_ref
    from pairwise_sample_optimization_amd import _lib
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    cuda, elem = torch.device("cuda:0"), _lib.ELEM_DTYPE
    cfg = UNetConfig.tiny(16) if which == "tiny16" else UNetConfig.sdxl(32)
    unet = UNet2DConditionModel(cfg).init_weights(0).to(cuda)
    g = torch.Generator(device="cuda").manual_seed(0)
    B, h = 2, cfg.sample_size
    sample = torch.randn(B, 4, h, h, device=cuda, generator=g).to(elem).float()
    t = torch.tensor([999.0, 499.0], device=cuda)
    enc = torch.randn(B, 77, cfg.cross_attention_dim, device=cuda, generator=g).to(elem)
    text = torch.randn(B, cfg.text_embed_dim, device=cuda, generator=g).to(elem)
    tid = torch.tensor([[8 * h, 8 * h, 0, 0, 8 * h, 8 * h]] * B, device=cuda, dtype=torch.float32)
    G = torch.randn(sample.shape, device=cuda, generator=torch.Generator(device="cuda").manual_seed(5))
    sd = sdxl_ref.sd_to(unet.state_dict(), cuda)
    ocfg = dict(time_proj_dim=cfg.time_proj_dim, addition_time_embed_dim=cfg.addition_time_embed_dim)
    oracle = lambda sd_, lora_: sdxl_ref.unet_forward(sd_, sample, t, enc.float(), text.float(), tid, lora=lora_,
                                                      cfg=ocfg)

    def hip():
        unet.lora.grad.zero_()
        out = unet(sample, t, enc, added_cond_kwargs={"text_embeds": text, "time_ids": tid}).sample
        ((out * G).sum() * loss_scale).backward()
        return out.detach(), {k: v.clone() / loss_scale for k, v in unet.lora.grad_dict_peft().items()}

    # plain LoRA: the HIP path's error, and the oracle's eps / gradients that DoRA has to move away from
    unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r))
    unet.lora.init_gaussian(seed=1, b_std=0.05)
    out_l, g_l = hip()
    lora = {k: v.float() for k, v in unet.lora.state_dict_peft().items()}
    leaf = {k: v.clone().requires_grad_(True) for k, v in lora.items()}
    e_l = oracle(sd, leaf)
    (e_l * G).sum().backward()
    gl32 = {k: v.grad for k, v in leaf.items()}
    res = SimpleNamespace(unet=unet, sample=sample, t=t, enc=enc, text=text, tid=tid, G=G, which=which, r=r)
    res.lora_eps, res.lora_grad = _rel(out_l, e_l), total_rel(g_l, gl32)
    # DoRA on the same UNet: same A / B, magnitudes spread around n
    st = unet.add_adapter(SimpleNamespace(r=r, lora_alpha=r, use_dora=True), allow_dora=True)
    st.init_gaussian(seed=1, b_std=0.05)
    now = st.state_dict_peft()
    assert all(torch.equal(now[k].float(), v) for k, v in lora.items()), "the two adapters must share A and B"
    n = norms(sd, lora, st.scale)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for p, v in n.items():
        st.magnitude_view(st.master, p).copy_(spread(v, gen, WIDTHS[which]))
    st.refresh()
    out_d, g_d = hip()
    leaf = {k: v.clone().requires_grad_(True) for k, v in lora.items()}
    mags = {p: st.magnitude_view(st.master, p).clone().requires_grad_(True) for p in n}
    e_d = oracle(*fold(sd, leaf, mags, st.scale))
    (e_d * G).sum().backward()
    gd32 = {k: v.grad for k, v in leaf.items()}
    gd32.update({f"{p}.{MAG}.weight": m.grad for p, m in mags.items()})
    mkeys = [k for k in gd32 if MAG in k]
    res.mine, res.ref, res.mkeys, res.out, res.eps32 = g_d, gd32, mkeys, out_d, e_d.detach()
    res.dora_eps, res.dora_grad, res.mag_grad = _rel(out_d, e_d), total_rel(g_d, gd32), total_rel(g_d, gd32, mkeys)
    # what the oracle alone says about the case: how far DoRA moves eps and the A / B gradients
    res.moved_eps, res.moved_grad = _rel(e_d, e_l), total_rel(gd32, gl32, list(gl32))
    print(f"\n  {which} r={r}: oracle DoRA vs LoRA: eps {res.moved_eps:.3e}  A/B grads {res.moved_grad:.3e}"
          f"\n  {which} r={r}: eps  DoRA {res.dora_eps:.3e}  plain LoRA {res.lora_eps:.3e}"
          f"\n  {which} r={r}: grads DoRA {res.dora_grad:.3e} (magnitudes alone {res.mag_grad:.3e})  plain LoRA "
          f"{res.lora_grad:.3e}  ({len(gd32)} tensors)", flush=True)
    return res
