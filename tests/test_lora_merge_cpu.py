"""CPU checks of merged-weight LoRA inference (fuse_lora): the C entry is declared, exported and bound; the Python
record of kernels.LoraMergeTable is the struct of csrc/lora_merge.hip; pso_lora_merge refuses bad tables before any
launch; the fp64 restatement's bound behaves; the trainers' opt-in defaults to off."""
import inspect
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import lora_merge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry():
    from pairwise_sample_optimization_amd import _lib
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"int\s+pso_lora_merge\(([^)]*)\);", h)
    assert m, "include/pso_amd.h does not declare pso_lora_merge"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["pso_lora_merge"][1]) == 4
    here = os.path.dirname(_lib.__file__)
    for so in ("libpso_amd.so", "libpso_amd_knobs.so", "libpso_amd_f16.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(here, so)]).decode()
        assert re.search(r" T pso_lora_merge$", out, flags=re.M), so
    assert _lib.lib().pso_lora_merge.restype is not None


def test_record_matches_the_struct():
    """Size and field offsets of kernels.LoraMergeTable's numpy record against struct LoraMergeDesc, laid out by the
    LP64 rules (pointers and long 8 bytes, int and float 4, natural alignment)."""
    import numpy as np
    from pairwise_sample_optimization_amd import kernels as K
    src = open(os.path.join(ROOT, "pairwise_sample_optimization_amd", "csrc", "lora_merge.hip")).read()
    body = re.search(r"struct LoraMergeDesc \{(.*?)\n\};", src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"((?:const\s+)?\w+\s*\*?)\s*(.*)$", decl, flags=re.S).groups()
        size = 8 if "*" in typ or typ.strip() == "long" else 4
        assert "*" in typ or typ.strip() in ("long", "int", "float"), typ
        fields += [(n.strip(), size) for n in names.split(",")]
    off, want = 0, {}
    for name, size in fields:
        off = -(-off // size) * size
        want[name] = off
        off += size
    total = -(-off // 8) * 8
    dt = np.dtype(K.LoraMergeTable.DTYPE)
    assert total == dt.itemsize == K.LoraMergeTable.RECORD == 72
    assert [n for n, _ in fields] == list(dt.names) == ["W", "A", "B", "g", "O", "ldw", "ldo", "out", "in", "r", "s"]
    assert {n: dt.fields[n][1] for n in dt.names} == want
    assert all(dt.fields[n][0].itemsize == size for n, size in fields)


_ARG_PROBE = """
import numpy as np
import torch
from pairwise_sample_optimization_amd import _lib, kernels as K
assert not torch.cuda.is_available()
l = _lib.lib()
dt = np.dtype(K.LoraMergeTable.DTYPE)
DEV = 0x70000                          # fake, never dereferenced: every case below fails a check before any launch
ok = dict(W=0x10000, A=0x20000, B=0x30000, g=0, O=0x40000, ldw=320, ldo=328, out=64, r=8, s=0.5)
ok["in"] = 320
def call(n, recs, dev=DEV, host=True):
    arr = np.zeros(max(len(recs), 1), dtype=dt)
    for i, rec in enumerate(recs):
        arr[i] = tuple(rec[k] for k in dt.names)
    return l.pso_lora_merge(n, dev, arr.ctypes.data if host else None, None)
cases = [("null-table", lambda: call(1, [ok], dev=None)), ("null-host", lambda: call(1, [ok], host=False)),
         ("n=0", lambda: call(0, [ok])), ("n<0", lambda: call(-3, [ok])), ("n>65535", lambda: call(65536, [ok]))]
for name, bad in [("in%4", {"in": 318}), ("W+2B", dict(W=0x10002)), ("W+4B", dict(W=0x10004)), ("O+4B", dict(O=0x40004)),
                  ("ldw%4", dict(ldw=322)), ("ldo%4", dict(ldo=330)), ("ldw<in", dict(ldw=316)),
                  ("ldo<in", dict(ldo=316)), ("A+8B", dict(A=0x20008)), ("A+4B", dict(A=0x20004)),
                  ("B+2B", dict(B=0x30002)), ("g+2B", dict(g=0x50002)), ("null-W", dict(W=0)), ("null-A", dict(A=0)),
                  ("null-B", dict(B=0)), ("null-O", dict(O=0)), ("out=0", dict(out=0)), ("r=0", dict(r=0))]:
    cases.append((name, lambda bad=bad: call(1, [dict(ok, **bad)])))
    cases.append(("second:" + name, lambda bad=bad: call(2, [ok, dict(ok, **bad)])))   # every record is checked
for name, fn in cases:
    rc = fn()
    print("case", name, rc, l.pso_last_error().decode())
"""


def test_entry_rejects_bad_tables_before_any_launch():
    """pso_lora_merge loads W and stores O 8 bytes at a time and loads A 16 bytes at a time; it reads the host copy
    of the table and refuses a record that breaks a rule with PSO_ERR_ARG and a message naming it, in all three
    library builds.  Host-only, like the probes of tests/test_abi.py: with a GPU present a regression would launch
    on the fake pointers, so the test skips itself there."""
    if torch.cuda.is_available():
        pytest.skip("argument checks are exercised where no launch can follow a regression (no GPU)")
    for pso_lib in (None, "knobs", "f16"):
        env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
        if pso_lib:
            env["PSO_LIB"] = pso_lib
        r = subprocess.run([sys.executable, "-c", _ARG_PROBE], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (pso_lib, r.stdout[-2000:] + r.stderr[-2000:])
        got = {m.group(1): (int(m.group(2)), m.group(3))
               for m in re.finditer(r"^case (\S+) (-?\d+) (.*)$", r.stdout, flags=re.M)}
        assert len(got) == 5 + 2 * 18, (pso_lib, r.stdout)
        for name, (rc, msg) in got.items():
            assert rc == 1, (pso_lib, name, rc, msg)  # PSO_ERR_ARG
            assert msg.startswith("pso_lora_merge: "), (pso_lib, name, msg)
            base = name.split(":")[-1]
            if name.startswith("second:"):
                assert "record 1:" in msg, (pso_lib, name, msg)
            if base in ("in%4", "W+2B", "W+4B", "O+4B", "ldw%4", "ldo%4", "ldw<in", "ldo<in"):
                assert "8-B aligned rows" in msg, (pso_lib, name, msg)
            elif base in ("A+8B", "A+4B", "B+2B", "g+2B"):
                assert "16-B boundary" in msg, (pso_lib, name, msg)
            else:
                assert "bad args" in msg, (pso_lib, name, msg)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ulp16_is_the_spacing_of_the_element_type(dtype):
    x = torch.tensor([1.0, 1.5, 1.999, 2.0, 0.75, 3e-3, 100.0], dtype=torch.float64)
    up = torch.nextafter(x.to(dtype), torch.tensor(float("inf"), dtype=dtype)).double() - x.to(dtype).double()
    assert torch.equal(R.ulp16(x.to(dtype).double(), dtype), up)
    tiny = torch.tensor([0.0, 1e-9], dtype=torch.float64)
    if dtype == torch.float16:  # below the smallest normal the spacing stays 2^-24
        assert torch.equal(R.ulp16(tiny, dtype), torch.full((2,), 2.0 ** -24, dtype=torch.float64))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("use_g", [False, True])
def test_bound_admits_fp32_arithmetic_and_refuses_a_dropped_term(dtype, use_g):
    """The formula evaluated in fp32 in the kernel's order and rounded once sits inside the bound; the same without
    the scale, without g, or from 16-bit-rounded A / B does not."""
    g0 = torch.Generator().manual_seed(5)
    out, fin, r, s = 33, 64, 8, 0.35
    W = (torch.randn(out, fin, generator=g0) * fin ** -0.5).to(dtype)
    A, B = torch.randn(r, fin, generator=g0) / r, torch.randn(out, r, generator=g0) * 0.1
    g = torch.exp2(torch.rand(out, generator=g0) * 2 - 1) if use_g else None
    v = torch.zeros(out, fin)
    for k in range(r):
        v = v + B[:, k:k + 1] * A[k:k + 1]
    e = W.float() + torch.tensor(s, dtype=torch.float32) * v
    if use_g:
        e = e * g[:, None]
    assert R.worst(e.to(dtype), W, A, B, s, g, dtype)[0] <= 1.0
    assert R.worst((W.float() + v).to(dtype), W, A, B, s, g, dtype)[1] > 0           # s dropped
    if use_g:
        assert R.worst((W.float() + s * v).to(dtype), W, A, B, s, g, dtype)[1] > 0   # g dropped
    lo = W.float() + s * (B.to(dtype).float() @ A.to(dtype).float())                 # the 16-bit working copies
    assert R.worst((lo * g[:, None] if use_g else lo).to(dtype), W, A, B, s, g, dtype)[1] > 0


# ----------------------------------------------------------------------------------------------------------------------
# the public surface
# ----------------------------------------------------------------------------------------------------------------------
def test_fused_sampling_defaults_to_off():
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    p = inspect.signature(PSOTrainer.__init__).parameters["fused_sampling"]
    assert p.default is False
    seen = {}

    class Probe(PSOTrainer):
        def __init__(self, unet, **kw):
            seen.update(kw)

    train = dict(distilled_train_steps=1, beta=50.0, eps=0.1, learning_rate=1e-5, adam_beta1=0.9, adam_beta2=0.999,
                 adam_weight_decay=1e-6, adam_epsilon=1e-8, max_grad_norm=1.0, gradient_accumulation_steps=1,
                 batch_size=1)
    cfg = lambda **extra: SimpleNamespace(sample=SimpleNamespace(num_steps=2), mixed_precision="no",
                                          train=SimpleNamespace(**train, **extra))
    Probe.from_config(None, cfg())
    assert seen["fused_sampling"] is False
    Probe.from_config(None, cfg(fused_sampling=True))
    assert seen["fused_sampling"] is True


def _meta_unet():
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        return UNet2DConditionModel(UNetConfig.tiny(16))


def test_a_unet_starts_unfused_and_fuse_needs_an_adapter():
    unet = _meta_unet()
    assert unet.lora_fused is False and unet._merged is None
    with pytest.raises(ValueError, match="no LoRA adapter"):
        unet.fuse_lora()
    with pytest.raises(ValueError, match="no LoRA adapter"):
        unet.merge_and_unload()
    st = unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    assert st.merge_on is False and st._merge_table is None
    assert unet.unfuse_lora() is unet and unet.lora_fused is False
    dora = _meta_unet()
    dora.add_adapter(SimpleNamespace(r=8, lora_alpha=8, use_dora=True), allow_dora=True)
    with pytest.raises(ValueError, match="lora_scale"):
        dora.fuse_lora(lora_scale=0.5)
