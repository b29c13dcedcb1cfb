"""MI355X-native PSO (Pairwise Sample Optimization) hot path for timestep-distilled SDXL.

Host side mirrors the reference's Python surface (pso_pytorch.diffusers_patch, the config_sdxl_*_dpo ConfigDicts,
and the diffusers UNet2DConditionModel call/checkpoint interface); all arithmetic runs in libpso_amd.so (HIP, gfx950).
"""
__version__ = "0.1.0"


def compute_dtype():
    """torch dtype of the loaded library's 16-bit element type: torch.bfloat16 (libpso_amd.so) or torch.float16
    (libpso_amd_f16.so, PSO_LIB=f16).  Per process, like accelerate's `mixed_precision`."""
    from . import _lib
    return _lib.ELEM_DTYPE
