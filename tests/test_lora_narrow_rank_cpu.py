"""Host side of the LoRA ranks below 8 (diffusers' default rank 4), no GPU: the rank rule of check_lora_config, and on
a meta-device SDXL UNet the logical state -- peft's shapes, the optimizer's segments, the gradient units -- that the
optimizer, the all-reduce and the checkpoints see, beside the padded rank the kernels run at."""
from types import SimpleNamespace

import pytest
import torch

NARROW = (1, 3, 4, 7)


@pytest.fixture(scope="module")
def states():
    """rank -> (unet, LoraState) on the meta device (full SDXL topology, nothing allocated)."""
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    out = {}
    for k in NARROW + (8,):
        with torch.device("meta"):
            unet = UNet2DConditionModel(UNetConfig.sdxl())
        out[k] = (unet, unet.add_adapter(SimpleNamespace(r=k, lora_alpha=k)))
    return out


@pytest.mark.parametrize("k", NARROW)
def test_add_adapter_accepts_narrow_ranks_with_peft_shapes(states, k):
    unet, st = states[k]
    assert st is unet.lora and st.r == k and st.scale == 1.0
    assert st.r_pad % 8 == 0 and st.r_pad >= k
    sd = st.state_dict_peft()
    names = list(st.adapter_names())
    assert len(names) == 70 * 8 and len(sd) == 2 * len(names)
    for name in names:
        A, B = sd[f"{name}.lora_A.weight"], sd[f"{name}.lora_B.weight"]
        blk = unet.get_submodule(name.rsplit(".attn", 1)[0])
        cross = ".attn2." in name and name.endswith((".to_k", ".to_v"))
        fin = blk.attn2.kv_dim if cross else blk.dim
        assert tuple(A.shape) == (k, fin), (name, A.shape)
        assert tuple(B.shape) == (blk.dim, k), (name, B.shape)
    # the flat logical buffers hold exactly these tensors: no pads
    assert st.master.numel() == st.grad.numel() == sum(v.numel() for v in sd.values())
    # the kernels' copies are the padded ones
    assert st.work.numel() == st.grad_pad.numel() == states[8][1].master.numel() * st.r_pad // 8


def test_rank4_master_is_half_of_rank8(states):
    assert 2 * states[4][1].master.numel() == states[8][1].master.numel()
    assert states[8][1].r_pad == 8 and states[8][1].grad_pad is None  # multiples of 8: one layout, no scratch
    assert states[8][1].work.numel() == states[8][1].master.numel()


@pytest.mark.parametrize("k", NARROW)
def test_trainable_segments_tile_the_logical_master(states, k):
    from pairwise_sample_optimization_amd.trainer import trainable_segments
    unet, st = states[k]
    segs = sorted(trainable_segments(unet))
    assert len(segs) == 70 * 16
    end = 0
    for off, n in segs:
        assert off == end, "gap or overlap between parameter tensors"
        end = off + n
    assert end == st.master.numel()
    if k == 4:
        # A [4][640] / B [640][4], the 1280-wide ones, and the cross-attention k / v A [4][2048]: the 640-wide tensors
        # are under bitsandbytes' 4096-element threshold (32-bit optimizer state), as peft's are
        assert {n for _, n in segs} == {2560, 5120, 8192}
        assert sum(n == 2560 for _, n in segs) > 0 and 2560 < 4096


@pytest.mark.parametrize("k", NARROW)
def test_grad_unit_ranges_tile_the_flat_gradient(states, k):
    unet, st = states[k]
    rng = unet.grad_unit_ranges()  # asserts that consecutive units are adjacent
    assert rng[0][1] == 0 and rng[-1][1] + rng[-1][2] == st.grad.numel()
    assert len(rng) == 11  # the attention-carrying units of the SDXL topology


@pytest.mark.parametrize("bad", [12, 0, 9, True, 4.0, -4])
def test_other_ranks_still_raise(bad):
    from pairwise_sample_optimization_amd.unet import check_lora_config
    with pytest.raises(ValueError, match="1..7 or a positive multiple of 8"):
        check_lora_config(SimpleNamespace(r=bad, lora_alpha=8))


def test_multiples_of_eight_and_narrow_ranks_pass_the_check():
    from pairwise_sample_optimization_amd.unet import check_lora_config
    for k in (1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64):
        assert check_lora_config(SimpleNamespace(r=k, lora_alpha=k)) == (k, k)
