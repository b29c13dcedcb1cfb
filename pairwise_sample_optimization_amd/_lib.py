"""ctypes binding of libpso_amd.so (the C-ABI declared in include/pso_amd.h).

The library is built in-tree by `make -C pairwise_sample_optimization_amd/csrc` (see __graft_entry__.build()).
There is NO fallback: if the shared object is missing or fails to load, every op raises.  torch is imported first so
that the HIP runtime torch ships (SONAME libamdhip64.so.7) is the one the library binds to.
"""
import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PSO_LIB=knobs selects the TOOLS build (libpso_amd_knobs.so: the same sources with the benchmark knobs of
# include/pso_amd_knobs.h compiled in) for A/B measurements and the knob-pinned kernel-form tests; the product path
# and everything else load libpso_amd.so, which has no knobs.  PSO_LIB_PATH: an explicit file (same-box A/B only).
# PSO_LIB=f16 selects libpso_amd_f16.so: the same sources with IEEE fp16 as the 16-bit element type (-DPSO_ELEM_F16,
# no knobs).  The element type is per process, as accelerate's `mixed_precision` is: one library, one ELEM_DTYPE.
KNOBS = os.environ.get("PSO_LIB", "") == "knobs"
F16 = os.environ.get("PSO_LIB", "") == "f16"
LIB_PATH = os.environ.get("PSO_LIB_PATH") or os.path.join(
    _HERE, "libpso_amd_knobs.so" if KNOBS else "libpso_amd_f16.so" if F16 else "libpso_amd.so")

PSO_F32 = 0
PSO_BF16 = 1
PSO_F16 = 2
# the library's 16-bit element type (checked against pso_elem_dtype() at load)
ELEM_DTYPE = torch.float16 if F16 else torch.bfloat16
ELEM_CODE = PSO_F16 if F16 else PSO_BF16
# image kinds of pso_clip_preprocess_img (include/pso_amd.h PSO_IMG_*): not dtype codes
IMG_F32, IMG_ELEM, IMG_U8 = 0, 1, 2
MODE_TURBO = 0
MODE_DMD = 1
MODE_DMD_F16 = 2   # DMD2 latent-dtype replay modes (include/pso_amd.h PSO_MODE_DMD_F16 / _BF16)
MODE_DMD_BF16 = 3
COEF_STRIDE = 8
# words of the device loss-scaler state (include/pso_amd.h PSO_AMP_*): floats and int32 counters, 4 bytes each
AMP_WORDS = 16
(AMP_SCALE, AMP_INV_SCALE, AMP_FOUND_INF, AMP_GROWTH_TRACKER, AMP_STEP, AMP_SKIPPED, AMP_NORM, AMP_CLIP_COEF,
 AMP_GRAD_MUL, AMP_BC1, AMP_BC2_SQRT, AMP_C1, AMP_C2) = range(13)
AMP_INT_WORDS = (AMP_FOUND_INF, AMP_GROWTH_TRACKER, AMP_STEP, AMP_SKIPPED)
# words of the Prodigy state block (include/pso_amd.h PSO_PRODIGY_*): the f64 fields span two 4-byte words each
PRODIGY_WORDS = 24
PRODIGY_F64 = {"d": 0, "d0": 2, "d_max": 4, "d_numerator": 6, "d_denom": 8, "d_hat": 10, "dlr": 12}
PRODIGY_I32 = {"k": 14, "updated": 15, "skipped": 16}
PRODIGY_DECOUPLE, PRODIGY_BIAS_CORRECTION, PRODIGY_SAFEGUARD_WARMUP = 1, 2, 4
# kinds of pso_lr_schedule (include/pso_amd.h PSO_LR_*): the --lr_scheduler names the DreamBooth script offers
LR_KINDS = {"constant": 0, "constant_with_warmup": 1, "linear": 2, "cosine": 3, "cosine_with_restarts": 4,
            "polynomial": 5}

_lib = None


class PsoTnRankProblem(ctypes.Structure):
    """include/pso_amd.h PsoTnRankProblem (one product of pso_gemm_tn_rank_batch)."""
    _fields_ = [("x", ctypes.c_void_p), ("ldx", ctypes.c_long), ("u", ctypes.c_void_p), ("ldu", ctypes.c_long),
                ("out", ctypes.c_void_p), ("ldo", ctypes.c_long), ("M", ctypes.c_int), ("C", ctypes.c_int),
                ("group_c", ctypes.c_int), ("alpha", ctypes.c_float)]

vp = ctypes.c_void_p
ci = ctypes.c_int
cf = ctypes.c_float
cd = ctypes.c_double
csz = ctypes.c_size_t
ci64 = ctypes.c_int64
cl = ctypes.c_long

# name -> (restype, argtypes).  Kept in sync with include/pso_amd.h (tests/test_abi.py checks every symbol).
SIGNATURES = {
    "pso_last_error": (ctypes.c_char_p, []),
    "pso_abi_version": (ci, []),
    "pso_elem_dtype": (ci, []),
    "pso_step_logprob_ws_bytes": (csz, [ci, ci]),
    "pso_step_logprob": (ci, [ci, ci, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, csz, vp]),
    "pso_pair_loss_ws_bytes": (csz, [ci, ci]),
    "pso_pair_loss_fwd": (ci, [ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, cf, cf, vp, vp, vp, csz, vp]),
    "pso_pair_loss_bwd": (ci, [ci, ci, ci, vp, vp, vp, ci, vp, vp, cf, cf, vp, cf, vp, ci, vp, csz, vp]),
    "pso_pair_loss_from_lp": (ci, [ci, ci, vp, vp, vp, cf, cf, vp, vp, vp]),
    "pso_db_loss_ws_bytes": (csz, [ci, ci]),
    "pso_db_loss_fwd": (ci, [ci, ci, ci, vp, vp, ci, vp, vp, vp, cf, cf, cf, vp, vp, vp, vp, csz, vp]),
    "pso_db_loss_bwd": (ci, [ci, ci, ci, vp, ci, vp, vp, vp, cf, cf, cf, vp, cf, vp, ci, vp, csz, vp]),
    "pso_gemm": (ci, [ci, ci, vp, cl, ci, vp, cl, vp, cl, ci, vp, cl, cf, vp, vp, cl, ci, vp, cl, vp, cl, ci, ci,
                      ci, ci, vp]),
    "pso_gemm_ws_bytes": (csz, [ci, ci, ci, ci]),
    "pso_gemm_ws": (ci, [ci, ci, vp, cl, ci, vp, cl, vp, cl, ci, vp, cl, cf, vp, vp, cl, ci, vp, cl, vp, cl, ci, ci,
                         ci, ci, vp, csz, vp]),
    "pso_gemm_batched": (ci, [ci, ci, ci, ci, vp, cl, cl, vp, cl, cl, cf, vp, cl, cl, ci, vp]),
    "pso_last_kernel": (ctypes.c_char_p, []),
    "pso_attention_small": (ci, [ci, ci, ci, ci, vp, cl, cl, vp, cl, cl, vp, cl, cl, ci, cf, vp, cl, cl, vp]),
    "pso_activation": (ci, [cl, vp, ci, vp]),
    "pso_embed_tokens": (ci, [ci, ci, ci, vp, vp, vp, vp, vp]),
    "pso_embed_vision": (ci, [ci, ci, ci, vp, vp, vp, vp, vp]),
    "pso_cosine_rows": (ci, [ci, ci, vp, cl, vp, cl, vp, vp]),
    "pso_row_mean": (ci, [ci, cl, vp, vp, vp]),
    "pso_patchify": (ci, [ci, ci, ci, ci, ci, vp, vp, vp]),
    "pso_clip_preprocess_ws_bytes": (csz, [ci, ci, ci, ci]),
    "pso_clip_preprocess": (ci, [ci, ci, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, csz, vp]),
    "pso_clip_preprocess_img": (ci, [ci, ci, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, csz, vp]),
    "pso_gemm_tn": (ci, [ci, ci, ci, vp, cl, vp, cl, cf, vp, cl, vp]),
    "pso_gemm_tn_grouped": (ci, [ci, ci, ci, vp, cl, vp, cl, cf, vp, cl, ci, vp]),
    "pso_gemm_tn_geglu": (ci, [ci, ci, ci, vp, cl, vp, cl, cf, vp, cl, vp]),
    "pso_gemm_tn_ws_bytes": (csz, [ci, ci, ci]),
    "pso_gemm_tn_ws": (ci, [ci, ci, ci, vp, cl, vp, cl, cf, vp, cl, vp, csz, vp]),
    "pso_gemm_tn_rank_batch": (ci, [ci, ci, ci, vp, vp]),
    "pso_gemm_tn_rank_batch_ws_bytes": (csz, [ci, ci, ci, vp]),
    "pso_gemm_tn_rank_batch_ws": (ci, [ci, ci, ci, vp, vp, csz, vp]),
    "pso_gemm_skinny_grouped": (ci, [ci, ci, ci, vp, cl, vp, cl, cf, vp, cl, ci, vp]),
    "pso_gemm_geglu": (ci, [ci, ci, vp, cl, ci, vp, cl, vp, vp, cl, vp, cl, ci, vp]),
    "pso_gemm_geglu_bwd": (ci, [ci, ci, vp, cl, ci, vp, cl, vp, cl, vp, cl, vp]),
    "pso_quant_rows_fp8": (ci, [ci, ci, vp, cl, vp, cl, vp, vp]),
    "pso_gemm_fp8": (ci, [ci, ci, ci, ci, vp, cl, vp, vp, cl, vp, vp, cl, ci, vp, vp, cl, vp, ci, ci, cf, vp, vp, cl,
                          vp, cl, vp, cl, ci, vp]),
    "pso_conv2d": (ci, [ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, cl, ci, vp, cl, cf, vp, vp,
                        cl, vp, cl, vp, cl, ci, ci, vp]),
    "pso_conv2d_ws_bytes": (csz, [ci, ci, ci, ci, ci, ci]),
    "pso_conv2d_ws": (ci, [ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, cl, ci, vp, cl, cf, vp, vp,
                           cl, vp, cl, vp, cl, ci, ci, vp, csz, vp]),
    "pso_group_norm_ws_bytes": (csz, [ci, ci, ci]),
    "pso_group_norm_fwd": (ci, [ci, ci, ci, ci, cf, vp, vp, vp, ci, vp, vp, vp, csz, vp]),
    "pso_group_norm_bwd": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, csz, vp]),
    "pso_layer_norm_fwd": (ci, [ci, ci, cf, vp, cl, vp, vp, vp, cl, vp, vp]),
    "pso_layer_norm_bwd": (ci, [ci, ci, vp, cl, vp, cl, vp, vp, vp, cl, vp, cl, vp]),
    "pso_attention_fwd": (ci, [ci, ci, ci, ci, vp, cl, cl, vp, cl, cl, vp, cl, cl, cf, vp, cl, cl, vp, vp]),
    "pso_attention_bwd_ws_bytes": (csz, [ci, ci, ci, ci]),
    "pso_attention_bwd": (ci, [ci, ci, ci, ci, vp, cl, cl, vp, cl, cl, vp, cl, cl, vp, cl, cl, vp, vp, cl, cl, cf,
                               vp, cl, cl, vp, cl, cl, vp, cl, cl, vp, csz, vp]),
    "pso_geglu_fwd": (ci, [cl, ci, vp, cl, vp, cl, vp]),
    "pso_geglu_bwd": (ci, [cl, ci, vp, cl, vp, cl, vp, cl, vp]),
    "pso_silu": (ci, [cl, vp, vp, vp]),
    "pso_timestep_embedding": (ci, [ci, ci, vp, vp, cl, ci, vp]),
    "pso_transpose": (ci, [ci, ci, ci, vp, cl, vp, cl, vp]),
    "pso_im2col3": (ci, [ci, ci, ci, ci, vp, vp, ci, vp]),
    "pso_colsum_acc": (ci, [cl, ci, vp, cl, cl, vp, cl, vp]),
    "pso_layer_norm_dparam": (ci, [ci, ci, vp, cl, vp, cl, vp, vp, vp, vp]),
    "pso_colsum_acc_ws_bytes": (csz, [cl, ci, cl]),
    "pso_colsum_acc_ws": (ci, [cl, ci, vp, cl, cl, vp, cl, vp, csz, vp]),
    "pso_layer_norm_dparam_ws_bytes": (csz, [ci, ci]),
    "pso_layer_norm_dparam_ws": (ci, [ci, ci, vp, cl, vp, cl, vp, vp, vp, vp, csz, vp]),
    "pso_im2col_conv": (ci, [ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, cl, vp]),
    "pso_sumpool2": (ci, [ci, ci, ci, ci, vp, vp, vp, vp]),
    "pso_axpby": (ci, [cl, cf, vp, cf, vp, vp, vp]),
    "pso_cast_f32_bf16": (ci, [cl, vp, cf, vp, vp]),
    "pso_cast_bf16_f32": (ci, [cl, vp, vp, vp]),
    "pso_conv_weight_t": (ci, [ci, ci, ci, ci, vp, vp, vp]),
    "pso_concat_channels": (ci, [cl, ci, vp, ci, vp, vp, vp]),
    "pso_nchw_to_nhwc": (ci, [ci, ci, ci, cl, vp, ci, cf, vp, vp]),
    "pso_softmax_rows": (ci, [ci, ci, vp, cl, vp]),
    "pso_grad_clip_ws_bytes": (csz, [cl]),
    "pso_transpose_batched": (ci, [ci, vp, ci, ci, vp]),
    "pso_transpose_multi": (ci, [ci, vp, ci, vp]),
    "pso_lora_pack": (ci, [ci, vp, cl, cf, vp]),
    "pso_lora_grad_fold": (ci, [ci, vp, cl, vp]),
    "pso_dora_weight_norm": (ci, [ci, vp, ci, ci, vp]),
    "pso_dora_scale_fwd": (ci, [ci, ci, ci, vp, cl, vp, vp, vp, cl, vp, cl, vp]),
    "pso_dora_bwd_ws_bytes": (csz, [ci, ci]),
    "pso_dora_bwd": (ci, [ci, ci, vp, cl, vp, cl, vp, vp, vp, cl, vp, vp, csz, vp]),
    "pso_lora_merge": (ci, [ci, vp, vp, vp]),
    "pso_gather_rows": (ci, [cl, cl, vp, vp, vp, vp]),
    "pso_grad_clip_coef": (ci, [cl, vp, cf, cf, vp, vp, csz, vp]),
    "pso_adamw_step": (ci, [cl, vp, vp, vp, vp, cf, vp, cf, cf, cf, cf, ci, cf, vp, vp, vp]),
    "pso_adamw8bit_blocks": (csz, [cl]),
    "pso_adamw8bit_maps": (None, [vp, vp]),
    "pso_adamw8bit_step": (ci, [cl, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cf, vp, cf, cf, cf, cf, ci, cf, vp,
                                vp, vp]),
    "pso_amp_unscale_clip": (ci, [cl, vp, cf, cf, cf, cf, vp, vp, csz, vp]),
    "pso_amp_update": (ci, [vp, cf, cf, ci, vp]),
    "pso_lr_schedule": (ci, [ci, cd, ci, ci, ci, cd, vp, ci, vp, vp]),
    "pso_prodigy_step_lr": (ci, [cl, vp, vp, vp, vp, vp, vp, vp, vp, cf, cf, cf, cf, cf, ci, cf, cf, cf, vp, vp, vp,
                                 csz, vp]),
    "pso_prodigy_ws_bytes": (csz, [cl]),
    "pso_prodigy_step": (ci, [cl, vp, vp, vp, vp, vp, vp, vp, cf, cf, cf, cf, cf, cf, ci, cf, cf, cf, vp, vp, vp, csz,
                              vp]),
    "pso_ema_step": (ci, [cl, vp, vp, cf, vp]),
    "pso_ema_swap": (ci, [cl, vp, vp, vp]),
    "pso_zero_f32": (ci, [cl, vp, vp]),
    "pso_preference": (ci, [ci, ci, vp, vp, ci, vp, vp]),
    "pso_nhwc_to_nchw": (ci, [ci, ci, cl, vp, vp, ci, vp]),
    "pso_split_channels": (ci, [cl, ci, ci, vp, vp, vp, vp, vp]),
}


class PsoGemmPlanQuery(ctypes.Structure):
    """include/pso_amd_knobs.h PsoGemmPlanQuery: a GEMM problem by value (alignments in bytes, 0 = operand absent)."""
    _fields_ = ([(n, ci) for n in ("variant", "group", "tn_split", "have_ws", "M", "N", "K1", "K2")] +
                [(n, cl) for n in ("lda1", "ldb1", "lda2", "ldb2")] +
                [(n, ci) for n in ("tail_group_n", "tail_rows", "batch", "out_dtype", "accumulate", "bias_align",
                                   "rowbias_align", "resid_align", "out_align")] +
                [(n, cl) for n in ("ld_rowbias", "ldr", "ldo")] + [("rows_per_group", ci), ("alpha", cf)] +
                [(n, ci) for n in ("conv_mode", "B", "C1", "C2", "H", "W", "Ho", "Wo", "ks", "stride", "pad",
                                   "tn_group")])


class PsoGemmPlanInfo(ctypes.Structure):
    """include/pso_amd_knobs.h PsoGemmPlanInfo: what csrc/gemm_plan.h decides."""
    _fields_ = [(n, ci) for n in ("form", "bm", "bn", "wm", "wn", "stages", "pipe", "epi", "conv_mode", "atomic_ks",
                                  "ws_ks", "stage_epi", "vec_ok", "group_m")]


PLAN_GEMM, PLAN_CONV, PLAN_BATCHED, PLAN_GEGLU, PLAN_GEGLU_BWD, PLAN_TN, PLAN_TN_GEGLU = range(7)  # enum PsoGemmPlanKind

# include/pso_amd_knobs.h: bound only when the TOOLS build is loaded (PSO_LIB=knobs)
KNOB_SIGNATURES = {
    "pso_gemm_set_variant": (None, [ci]),
    "pso_gemm_plan_query": (ci, [ci, ctypes.POINTER(PsoGemmPlanQuery), ctypes.POINTER(PsoGemmPlanInfo)]),
    "pso_gemm8p_skip_epilogue": (None, [ci]),
    "pso_gemm_tn_set_split": (None, [ci]),
    "pso_attention_set_variant": (None, [ci]),
    "pso_attn_pp_trace": (ci, [vp]),
}


class PsoLibError(RuntimeError):
    pass


def _bind(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if KNOBS:
        for name, (res, args) in KNOB_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args


def require_knobs(what):
    """The benchmark knobs exist in the TOOLS build only (include/pso_amd_knobs.h)."""
    if not KNOBS:
        raise PsoLibError(f"{what} is a benchmark knob: run with PSO_LIB=knobs (libpso_amd_knobs.so); the product "
                          "library libpso_amd.so has none")


def require_bf16(what):
    """Paths that were verified against their oracles in bf16 only raise under the f16 library instead of running
    unverified: the fp8 forward, full-UNet training (clip.py has an opt-in: require_bf16_or_opt_in)."""
    if F16:
        raise PsoLibError(f"{what} is not supported by the f16 library (PSO_LIB=f16, libpso_amd_f16.so): unset "
                          "PSO_LIB and run it on the bf16 library")


def require_bf16_or_opt_in(what, allow_f16):
    """The CLIP towers and their image path (clip.py, kernels.clip_preprocess): refused under the f16 library unless
    the caller opts in with allow_f16=True -- the default refusal is part of that library's contract.  Under a bf16
    library the keyword changes nothing."""
    if F16 and not allow_f16:
        raise PsoLibError(f"{what} is not supported by the f16 library (PSO_LIB=f16, libpso_amd_f16.so) by default: "
                          "pass allow_f16=True to run it in fp16, or unset PSO_LIB and run it on the bf16 library")


def lib():
    """Load (once) and return the bound library; raises if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PsoLibError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(no CPU fallback exists)")
        l = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        _bind(l)
        if l.pso_elem_dtype() != ELEM_CODE:
            raise PsoLibError(f"{LIB_PATH} has 16-bit element code {l.pso_elem_dtype()}, but PSO_LIB="
                              f"{os.environ.get('PSO_LIB', '')!r} expects {ELEM_CODE} ({ELEM_DTYPE}): PSO_LIB=f16 goes "
                              "with libpso_amd_f16.so, everything else with a bf16 library")
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().pso_last_error().decode(errors="replace")
        raise PsoLibError(f"{what} failed (rc={rc}): {msg}")


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dtype_code(t):
    if t.dtype == torch.float32:
        return PSO_F32
    if t.dtype == ELEM_DTYPE:
        return ELEM_CODE
    if t.dtype in (torch.float16, torch.bfloat16):
        raise PsoLibError(f"{t.dtype} tensor, but the loaded library's 16-bit element type is {ELEM_DTYPE} "
                          f"({os.path.basename(LIB_PATH)}): " + ("unset PSO_LIB for the bf16 library" if F16 else
                          "set PSO_LIB=f16 for libpso_amd_f16.so") + "; the element type is per process")
    raise PsoLibError(f"unsupported dtype {t.dtype}")


def require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise PsoLibError("libpso_amd ops take device tensors only (no CPU fallback)")
