"""The cases of the GEMM dispatch table (tests/golden/gemm_dispatch_table.json, tests/test_gemm_plan_cpu.py).

Pure Python, no torch.  cases() lists, in a fixed order, the problems whose kernel choice is pinned: each is a dict
with the entry point ("entry"), the variant, and the fields of include/pso_amd_knobs.h PsoGemmPlanQuery that differ
from DEFAULTS (row pitches default to the dense ones, pointers to 16-byte alignment).  plan_of_kernel() turns a noted
kernel name (pso_last_kernel) into the same fields plan_of_info() takes from a PsoGemmPlanInfo, so a recorded launch
and a queried plan compare with ==.
"""
import re

PSO_F32, ELEM = 0, 1
CONV_NORMAL, CONV_UP2 = 1, 2
PLAN_GEMM, PLAN_CONV, PLAN_BATCHED, PLAN_GEGLU, PLAN_GEGLU_BWD, PLAN_TN, PLAN_TN_GEGLU = range(7)
KIND = {"pso_gemm": PLAN_GEMM, "pso_gemm_ws": PLAN_GEMM, "pso_conv2d": PLAN_CONV, "pso_conv2d_ws": PLAN_CONV,
        "pso_gemm_batched": PLAN_BATCHED, "pso_gemm_geglu": PLAN_GEGLU, "pso_gemm_geglu_bwd": PLAN_GEGLU_BWD,
        "pso_gemm_tn": PLAN_TN, "pso_gemm_tn_grouped": PLAN_TN, "pso_gemm_tn_ws": PLAN_TN, "pso_gemm_tn_geglu": PLAN_TN_GEGLU}
# every variant number in use (include/pso_amd_knobs.h enum PsoGemmVariant)
VARIANTS = [v for v in range(1, 59) if v not in (9, 13, 15, 53, 54)]
DEFAULTS = dict(variant=0, group=0, tn_split=0, have_ws=0, M=0, N=0, K1=0, K2=0, lda1=None, ldb1=None, lda2=None,
                ldb2=None, tail_group_n=0, tail_rows=0, batch=0, out_dtype=ELEM, accumulate=0, bias_align=0,
                rowbias_align=0, resid_align=0, out_align=16, ld_rowbias=None, ldr=None, ldo=None, rows_per_group=0,
                alpha=1.0, conv_mode=0, B=0, C1=0, C2=0, H=0, W=0, Ho=0, Wo=0, ks=0, stride=0, pad=0, tn_group=0)


def full(case):
    """The case with every query field set (dense row pitches where none is given)."""
    c = dict(DEFAULTS, **{k: v for k, v in case.items() if k != "entry"})
    kind = KIND[case["entry"]]
    c["have_ws"] = int(case["entry"].endswith("_ws"))
    if kind == PLAN_CONV:
        c["M"], c["K1"] = c["B"] * c["Ho"] * c["Wo"], c["ks"] * c["ks"] * (c["C1"] + c["C2"])
    if kind in (PLAN_TN, PLAN_TN_GEGLU):  # M reduction rows, N = I, K1 = J: operands [M][I] and [M][J]
        dense = dict(lda1=c["N"], ldb1=c["K1"])
    else:
        groups = c["N"] // c["tail_group_n"] if c["tail_group_n"] else 1
        dense = dict(lda1=c["K1"], ldb1=c["K1"], lda2=c["K2"] * groups, ldb2=c["K2"], ld_rowbias=c["N"], ldr=c["N"],
                     ldo=c["N"] // 2 if kind == PLAN_GEGLU else 2 * c["N"] if kind == PLAN_GEGLU_BWD else c["N"])
    for k, v in dense.items():
        if c[k] is None:
            c[k] = v
    return {k: (0 if v is None else v) for k, v in c.items()}


def _dense(entry, M, N, K1, tail, epi, f32, **more):
    c = dict(entry=entry, M=M, N=N, K1=K1, **more)
    if tail:
        c.update(K2=tail, tail_group_n=N // 3 if tail == 96 else 0)
    if epi:
        c.update(bias_align=16, resid_align=16)
    if f32:
        c.update(out_dtype=PSO_F32, accumulate=1)
    return c


def _conv(entry, variant, B, C1, H, Cout, mode=CONV_NORMAL, stride=1, C2=0, up=1, **more):
    Ho = H * up // stride
    return dict(entry=entry, variant=variant, conv_mode=mode, B=B, C1=C1, C2=C2, H=H, W=H, Ho=Ho, Wo=Ho, ks=3,
                stride=stride, pad=1, N=Cout, bias_align=16, **more)


def cases():
    out = []
    # dense pso_gemm / pso_gemm_ws, automatic dispatch.  The workspace entry leaves out M = 65536 (512 row tiles: far
    # beyond any split plan), which keeps the table within 20 000 cases.
    Ms = (64, 256, 1024, 2048, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 65536)
    Ns = (32, 64, 96, 128, 256, 320, 640, 1280, 1920, 2560, 3840, 5120, 10240)
    Ks = (320, 640, 1280, 2560, 5120, 10240)
    for entry in ("pso_gemm", "pso_gemm_ws"):
        for M in Ms[:-1] if entry == "pso_gemm_ws" else Ms:
            for N in Ns:
                for K1 in Ks:
                    for tail in (0, 32, 96):
                        if tail == 96 and N % (3 * 64):
                            continue
                        for epi in (0, 1):
                            for f32 in (0, 1):
                                out.append(_dense(entry, M, N, K1, tail, epi, f32))
    # the two alignment breakers: output rows that are not 16-byte multiples, A and B pitches that differ
    for M in (4096, 16384):
        for N in (640, 1280, 2560):
            for K1 in (640, 5120):
                for epi in (0, 1):
                    out.append(_dense("pso_gemm", M, N, K1, 0, epi, 0, ldo=N + 4, ldr=N + 4))
                    out.append(_dense("pso_gemm", M, N, K1, 0, epi, 0, lda1=K1 + 8))
    # every variant on a reduced grid
    for variant in VARIANTS:
        for M in (2048, 4096, 16384, 65536):
            for N in (640, 1280, 2560, 5120):
                for K1 in (640, 5120):
                    for tail in (0, 32):
                        out.append(_dense("pso_gemm", M, N, K1, tail, 0, 0, variant=variant))
    # convolutions: the UNet's 3x3 shapes at 1, 2 and 8 images; stride 2, the fused 2x upsample, two channel sources,
    # and the VAE decoder's conv_out to RGB (the direct small-Cout kernel, pso_conv2d only)
    for entry in ("pso_conv2d", "pso_conv2d_ws"):
        for variant in (0, 43, 44, 52):
            for B in (1, 2, 8):
                for C in (320, 640, 1280, 1920, 2560):
                    for H in (32, 64, 128):
                        out.append(_conv(entry, variant, B, C, H, C))
            out.append(_conv(entry, variant, 2, 320, 128, 320, stride=2))
            out.append(_conv(entry, variant, 2, 640, 32, 640, mode=CONV_UP2, up=2))
            out.append(_conv(entry, variant, 2, 640, 64, 640, C2=640, rowbias_align=16, resid_align=16))
            out.append(_conv(entry, variant, 1, 128, 64, 3))
    # GEGLU forward (N = 2 F interleaved columns) and backward (N = F) at the three SDXL-style widths
    for variant in (0, 31, 45, 57, 58):
        for M in (2048, 4096, 6144, 8192, 16384, 32768, 65536):
            for dim in (320, 640, 1280):
                out.append(dict(entry="pso_gemm_geglu", variant=variant, M=M, N=8 * dim, K1=dim, bias_align=16))
                out.append(dict(entry="pso_gemm_geglu_bwd", variant=variant, M=M, N=4 * dim, K1=dim))
    # batched (the VAE's mid attention): either side of the 256-tile thresholds of the 128 x 160 and 128 x 128 tiles
    for batch, M, N, K in ((1, 4096, 4096, 512), (1, 1024, 1024, 512), (4, 1024, 1024, 512), (1, 4096, 640, 4096),
                           (2, 4096, 640, 4096), (1, 4096, 1280, 4096)):
        out.append(dict(entry="pso_gemm_batched", batch=batch, M=M, N=N, K1=K))
    # TN products (M reduction rows; N = I, K1 = J)
    for variant in (0, 56):
        tn = []
        for M in (4096, 16384):  # the LoRA shapes, either side the rank
            for wide in (640, 1280):
                for r in (16, 32, 64, 96):
                    tn += [(M, wide, r), (M, r, wide)]
        # the full-weight shapes (csrc/gemm_plan.h, above tn256_slices and tn128_atomic_slices)
        tn += [(6144, 1280, 11520), (24576, 1280, 11520), (6144, 10240, 1280), (6144, 3840, 1280), (6144, 1280, 5120),
               (6144, 1280, 1280), (24576, 640, 640), (98304, 320, 2880)]
        for entry in ("pso_gemm_tn", "pso_gemm_tn_ws"):
            out += [dict(entry=entry, variant=variant, M=M, N=I, K1=J) for M, I, J in tn]
        for M in (4096, 16384):  # grouped q/k/v: 3 x 1280 columns against 3 x r
            for r in (16, 32, 64, 96):
                out.append(dict(entry="pso_gemm_tn_grouped", variant=variant, M=M, N=3840, K1=3 * r, tn_group=1280))
        for M, F2, J in ((6144, 10240, 1280), (16384, 5120, 640), (4096, 10240, 1280)):
            out.append(dict(entry="pso_gemm_tn_geglu", variant=variant, M=M, N=F2, K1=J))
    return out


# gemm_plan.h GemmForm / TnKind -> the family a kernel name shows
_FORM = {1: "tile", 2: "8p", 3: "8p", 4: "8p", 5: "8p", 6: "skinny", 7: "small_conv"}
_TN = {1: "tn_rank", 2: "tn128", 3: "tn64", 4: "tn256"}
PLAN_FIELDS = ("family", "bm", "bn", "wm", "wn", "stages", "pipe", "conv", "epi", "ws_ks")


def _plan(family, bm=0, bn=0, wm=0, wn=0, stages=0, pipe=0, conv=0, epi=0, ws_ks=0):
    if family in ("skinny", "tn_rank"):  # their inner choice is gemm_skinny.hip's / gemm_tn_rank.hip's
        ws_ks = 0
    return [family, bm, bn, wm, wn, stages, pipe, conv, epi, ws_ks]


def plan_of_kernel(name, ws_ks=0):
    """The plan fields a noted kernel name shows; ws_ks = the workspace split count of the call (0: not split)."""
    m = re.fullmatch(r"gemm_bf16_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false), (\d+)>", name)
    if m:
        bm, bn, conv, wm, wn, st = (int(x) for x in m.groups()[:6])
        return _plan("tile", bm, bn, wm, wn, st, int(m.group(7) == "true"), conv, int(m.group(8)), ws_ks)
    m = re.fullmatch(r"gemm8p_kernel<(\d), true, false, false, (\d+), (true|false)>", name)
    if m:
        return _plan("8p", bn=int(m.group(2)), conv=int(m.group(3) == "true"), epi=int(m.group(1)))
    for prefix, family in (("gemm_skinny_nt_kernel<", "skinny"), ("conv3x3_smallc_kernel<", "small_conv"),
                           ("gemm_tn_rank_kernel<", "tn_rank"), ("gemm_tn256_kernel", "tn256"),
                           ("gemm_tn128_kernel", "tn128"), ("gemm_tn_kernel", "tn64")):
        if name.startswith(prefix):
            return _plan(family, ws_ks=ws_ks)
    raise ValueError(f"unknown kernel name {name!r}")


def plan_of_info(kind, info):
    """The same fields from a PsoGemmPlanInfo (any object with its attributes)."""
    if kind in (PLAN_TN, PLAN_TN_GEGLU):
        return _plan(_TN[info.form], ws_ks=info.ws_ks)
    family = _FORM[info.form]
    if family == "tile":
        return _plan("tile", info.bm, info.bn, info.wm, info.wn, info.stages, info.pipe, info.conv_mode, info.epi,
                     info.ws_ks)
    if family == "8p":
        return _plan("8p", bn=info.bn, conv=int(info.form == 5), epi=info.epi)
    return _plan(family)
