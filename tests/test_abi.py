"""CPU checks of the C-ABI boundary: the library builds/loads and exports every symbol include/pso_amd.h declares
(no compute calls: there is no GPU here)."""
import os
import glob
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\**\s+\**(pso_\w+)\(", h, flags=re.M)))


def test_header_declares_functions():
    names = _declared()
    assert "pso_gemm" in names and "pso_pair_loss_fwd" in names and "pso_attention_bwd" in names
    assert len(names) >= 25


def test_library_exports_every_declared_symbol():
    from pairwise_sample_optimization_amd import _lib
    l = _lib.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pso_\w+)", out))
    for name in _declared():
        assert name in exported, name
        assert name in _lib.SIGNATURES, f"{name} not bound in _lib.SIGNATURES"
        getattr(l, name)
    assert l.pso_abi_version() == 2


def test_bound_signatures_match_header_arity():
    from pairwise_sample_optimization_amd import _lib
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for m in re.finditer(r"(pso_\w+)\(([^)]*)\);", h):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert len(_lib.SIGNATURES[name][1]) == n, (name, n, len(_lib.SIGNATURES[name][1]))


def test_no_cpu_fallback():
    import pytest
    import torch
    from pairwise_sample_optimization_amd import kernels, _lib
    a = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.PsoLibError):
        kernels.gemm(a, a)


_ATTN_BWD_ARG_PROBE = """
import torch
from pairwise_sample_optimization_amd import _lib
assert not torch.cuda.is_available()
l = _lib.lib()
B, H, Sq, Sk, C = 2, 5, 300, 77, 320   # the short-key backward with 5 query splits
assert l.pso_attention_bwd_ws_bytes(B, H, Sq, Sk) > 2 * 256 * -(-(B * H * Sq * 4) // 256)
IN = 0x10000                            # fake, never dereferenced: every case below fails a check before any launch
ok = dict(dq=0x20000, lddq=C, sdq_b=Sq * C, dk=0x30000, lddk=C, sdk_b=Sk * C, dv=0x40000, lddv=C, sdv_b=Sk * C)
cases = [("dq+4B", dict(dq=0x20004)), ("dk+4B", dict(dk=0x30004)), ("dv+4B", dict(dv=0x40004)),
         ("lddq%4", dict(lddq=C + 2, sdq_b=Sq * (C + 2))), ("lddk%4", dict(lddk=C + 2, sdk_b=Sk * (C + 2))),
         ("lddv%4", dict(lddv=C + 2, sdv_b=Sk * (C + 2))),
         ("sdk_b", dict(sdk_b=(Sk + 3) * C)), ("sdv_b", dict(sdv_b=(Sk + 3) * C))]
for name, bad in cases:
    a = dict(ok, **bad)
    rc = l.pso_attention_bwd(B, H, Sq, Sk, IN, C, Sq * C, IN, C, Sk * C, IN, C, Sk * C, IN, C, Sq * C, IN, IN, C,
                             Sq * C, 0.125, a["dq"], a["lddq"], a["sdq_b"], a["dk"], a["lddk"], a["sdk_b"], a["dv"],
                             a["lddv"], a["sdv_b"], IN, 1 << 40, None)
    print("case", name, rc, l.pso_last_error().decode())
"""


def test_attention_bwd_checks_output_alignment_and_split_batch_stride():
    """pso_attention_bwd stores dQ / dK / dV 8 bytes at a time, and its query-split reduction walks dK / dV as B * Sk
    rows of one stride: both are argument checks of the C entry point, in all three library builds.  Called with small
    fake addresses that break each rule in turn; every call must come back PSO_ERR_ARG with a message that names the
    rule (on a machine without a device a launch would return non-zero too: only the message tells them apart).
    Host-only on purpose: with a GPU present a regression would launch on the fake pointers, so the test skips itself
    there."""
    import sys
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("argument checks are exercised where no launch can follow a regression (no GPU)")
    for pso_lib in (None, "knobs", "f16"):
        env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
        if pso_lib:
            env["PSO_LIB"] = pso_lib
        r = subprocess.run([sys.executable, "-c", _ATTN_BWD_ARG_PROBE], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (pso_lib, r.stdout[-2000:] + r.stderr[-2000:])
        got = {m.group(1): (int(m.group(2)), m.group(3))
               for m in re.finditer(r"^case (\S+) (-?\d+) (.*)$", r.stdout, flags=re.M)}
        assert len(got) == 8, (pso_lib, r.stdout)
        for name, (rc, msg) in got.items():
            assert rc == 1, (pso_lib, name, rc, msg)  # PSO_ERR_ARG
            want = "dk/dv batch strides of Sk rows" if name.startswith("sd") else "dq/dk/dv need 8-B aligned rows"
            assert msg.startswith("pso_attention_bwd: ") and want in msg, (pso_lib, name, msg)


_LN_ARG_PROBE = """
import torch
from pairwise_sample_optimization_amd import _lib
assert not torch.cuda.is_available()
l = _lib.lib()
M, C = 5, 640
P = [0x10000 * (i + 1) for i in range(5)]   # fake, never dereferenced: every case fails a check before any launch
fwd = dict(x=P[0], ldx=C, gamma=P[1], beta=P[2], y=P[3], ldy=C)
for name, bad in [("x+8B", dict(x=P[0] + 8)), ("y+2B", dict(y=P[3] + 2)), ("gamma+8B", dict(gamma=P[1] + 8)),
                  ("beta+4B", dict(beta=P[2] + 4)), ("ldx%8", dict(ldx=C + 4)), ("ldy%8", dict(ldy=C + 12))]:
    a = dict(fwd, **bad)
    rc = l.pso_layer_norm_fwd(M, C, 1e-5, a["x"], a["ldx"], a["gamma"], a["beta"], a["y"], a["ldy"], P[4], None)
    print("case fwd:" + name, rc, l.pso_last_error().decode())
bwd = dict(x=P[0], ldx=C, dy=P[1], lddy=C, gamma=P[2], dadd=P[3], ldadd=C, dx=P[4], lddx=C)
for name, bad in [("x+8B", dict(x=P[0] + 8)), ("dy+8B", dict(dy=P[1] + 8)), ("gamma+2B", dict(gamma=P[2] + 2)),
                  ("dadd+8B", dict(dadd=P[3] + 8)), ("dx+4B", dict(dx=P[4] + 4)), ("ldx%8", dict(ldx=C + 4)),
                  ("lddy%8", dict(lddy=C + 4)), ("ldadd%8", dict(ldadd=C + 4)), ("lddx%8", dict(lddx=C + 2))]:
    a = dict(bwd, **bad)
    rc = l.pso_layer_norm_bwd(M, C, a["x"], a["ldx"], a["dy"], a["lddy"], 0x90000, a["gamma"], a["dadd"], a["ldadd"],
                              a["dx"], a["lddx"], None)
    print("case bwd:" + name, rc, l.pso_last_error().decode())
"""


def test_layer_norm_checks_row_alignment_of_every_operand():
    """pso_layer_norm_fwd / _bwd read and write every row as 16-byte chunks: a base pointer off a 16-byte boundary or
    an ld that is no multiple of 8 elements is refused with PSO_ERR_ARG and a message that names the rule, for each
    operand in turn (gamma, beta and dadd included), in all three library builds.  Host-only, like the attention
    probe above: with a GPU present a regression would launch on the fake pointers."""
    import sys
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("argument checks are exercised where no launch can follow a regression (no GPU)")
    for pso_lib in (None, "knobs", "f16"):
        env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
        if pso_lib:
            env["PSO_LIB"] = pso_lib
        r = subprocess.run([sys.executable, "-c", _LN_ARG_PROBE], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (pso_lib, r.stdout[-2000:] + r.stderr[-2000:])
        got = {m.group(1): (int(m.group(2)), m.group(3))
               for m in re.finditer(r"^case (\S+) (-?\d+) (.*)$", r.stdout, flags=re.M)}
        assert len(got) == 15, (pso_lib, r.stdout)
        for name, (rc, msg) in got.items():
            assert rc == 1, (pso_lib, name, rc, msg)  # PSO_ERR_ARG
            entry = "pso_layer_norm_fwd: " if name.startswith("fwd:") else "pso_layer_norm_bwd: "
            assert msg.startswith(entry) and "16-B aligned rows" in msg, (pso_lib, name, msg)


def test_product_library_has_no_benchmark_knobs():
    """the benchmark knobs (include/pso_amd_knobs.h) and the measured-not-kept kernel forms live in the
    tools build only.  The product library exports none of the knob setters, reads no environment variable, and holds
    no g_* dispatch state; the tools build exports every knob the header declares."""
    from pairwise_sample_optimization_amd import _lib
    prod = os.path.join(os.path.dirname(_lib.__file__), "libpso_amd.so")
    knobs = os.path.join(os.path.dirname(_lib.__file__), "libpso_amd_knobs.so")
    h = open(os.path.join(ROOT, "include", "pso_amd_knobs.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    knob_names = sorted(set(re.findall(r"^\s*\w+\s+\**(pso_\w+)\(", h, flags=re.M)))
    assert set(knob_names) == set(_lib.KNOB_SIGNATURES), knob_names
    exported = set(re.findall(r" T (pso_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", prod]).decode()))
    assert not (exported & set(knob_names)), exported & set(knob_names)
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", prod]).decode()
    assert "getenv" not in undefined
    local = subprocess.check_output(["nm", "-C", prod]).decode()
    assert not re.search(r" [bBdD] g_(gemm|tn|attn|skip|mode|grid)", local)
    assert "attn_bwd_dkv_pp_kernel" not in local
    kexp = set(re.findall(r" T (pso_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", knobs]).decode()))
    assert set(knob_names) <= kexp and set(_declared()) <= kexp
    for src in glob.glob(os.path.join(ROOT, "pairwise_sample_optimization_amd", "csrc", "*.hip")):
        txt = open(src).read()
        for m in re.finditer(r"^static (?:const )?(?:int|bool) g_\w+", txt, flags=re.M):
            # every mutable dispatch global sits inside an #ifdef PSO_BENCH_KNOBS block
            before = txt[:m.start()]
            assert before.rfind("#ifdef PSO_BENCH_KNOBS") > before.rfind("#endif"), (src, m.group(0))
