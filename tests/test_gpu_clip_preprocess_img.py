"""pso_clip_preprocess_img under the bf16 library: for every image type the old entry takes, the entry keyed by image
kind (kernels.clip_preprocess(..., allow_f16=True)) gives the old entry's bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8], ids=["bf16", "f32", "u8"])
def test_preprocess_img_equals_preprocess(cuda, dtype):
    from pairwise_sample_optimization_amd import kernels as K
    from pairwise_sample_optimization_amd.clip import CLIP_MEAN, CLIP_STD
    B, H, W, size = 2, 96, 72, 28
    g = torch.Generator(device="cuda").manual_seed(H + W)
    # smooth structure + noise + out-of-range values (clamped by the quantisation)
    yy, xx = torch.linspace(-1.2, 1.2, H, device=cuda), torch.linspace(-1.2, 1.2, W, device=cuda)
    img = (yy[None, :, None, None] * xx[None, None, :, None] * torch.randn(B, 1, 1, 3, device=cuda, generator=g)
           + 0.3 * torch.randn(B, H, W, 3, device=cuda, generator=g))
    if dtype == torch.uint8:
        img = ((img + 1.0) * 127.5).clamp(0, 255).to(torch.uint8)
    img = img.to(dtype).contiguous()
    old = K.clip_preprocess(img, size, 14, 592, CLIP_MEAN, CLIP_STD)
    new = K.clip_preprocess(img, size, 14, 592, CLIP_MEAN, CLIP_STD, allow_f16=True)
    assert new.dtype == old.dtype == torch.bfloat16 and tuple(new.shape) == (B * 4, 592)
    assert old.float().abs().max().item() > 0.5 and old.float().unique().numel() > 100  # a real image came through
    assert torch.equal(new, old), (new.float() - old.float()).abs().max().item()
