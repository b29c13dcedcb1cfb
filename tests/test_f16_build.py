"""The fp16 build of the kernels (libpso_amd_f16.so: every source with -DPSO_ELEM_F16) and fp16 mixed-precision
training's host pieces.

The 16-bit element type is fixed per library and per process (PSO_LIB=f16 selects the f16 library, as accelerate's
`mixed_precision` is per process), so everything that loads it runs in a child process.  The existing suite is NOT run
under PSO_LIB=f16: those tests build bf16 inputs, and their bit tests pin the bf16 library.  The f16 library's GPU cases
live in tests/test_gpu_f16.py, which skips itself unless PSO_LIB=f16; the one `gpu` test here runs it in a child."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pairwise_sample_optimization_amd")
F16_LIB = os.path.join(PKG, "libpso_amd_f16.so")


def _declared(header):
    h = open(os.path.join(ROOT, "include", header)).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\**\s+\**(pso_\w+)\(", h, flags=re.M)))


def test_f16_library_exports_the_abi_and_nothing_else():
    """Same nm checks as test_abi.py makes of the product library: every declared symbol, no knob setter, no getenv,
    no mutable dispatch global, none of the measured-not-kept kernel forms."""
    assert os.path.exists(F16_LIB), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    exported = set(re.findall(r" T (pso_\w+)",
                              subprocess.check_output(["nm", "-D", "--defined-only", F16_LIB]).decode()))
    names = _declared("pso_amd.h")
    assert "pso_elem_dtype" in names and len(names) >= 25
    for name in names:
        assert name in exported, name
    knobs = set(_declared("pso_amd_knobs.h"))
    assert knobs and not (exported & knobs), exported & knobs
    assert "getenv" not in subprocess.check_output(["nm", "-D", "--undefined-only", F16_LIB]).decode()
    local = subprocess.check_output(["nm", "-C", F16_LIB]).decode()
    assert not re.search(r" [bBdD] g_(gemm|tn|attn|skip|mode|grid)", local)
    assert "attn_bwd_dkv_pp_kernel" not in local


def _child(code, pso_lib):
    env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
    if pso_lib is not None:
        env["PSO_LIB"] = pso_lib
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


_PROBE = """
import torch
import pairwise_sample_optimization_amd as pkg
from pairwise_sample_optimization_amd import _lib
l = _lib.lib()
assert l.pso_abi_version() == 2
print("path", _lib.LIB_PATH)
print("elem", l.pso_elem_dtype())
print("compute", pkg.compute_dtype())
print("f32", _lib.dtype_code(torch.zeros(1)))
for dt in (torch.float16, torch.bfloat16):
    try:
        print("code", dt, _lib.dtype_code(torch.zeros(1, dtype=dt)))
    except _lib.PsoLibError as e:
        print("raises", dt, str(e).replace(chr(10), " "))
"""


def test_pso_lib_f16_selects_the_f16_library():
    out = _child(_PROBE, "f16")
    assert re.search(r"^path .*libpso_amd_f16\.so$", out, flags=re.M), out
    assert "elem 2\n" in out and "compute torch.float16\n" in out and "f32 0\n" in out, out
    assert "code torch.float16 2\n" in out, out
    m = re.search(r"^raises torch.bfloat16 (.*)$", out, flags=re.M)
    assert m and "PSO_LIB" in m.group(1), out  # the message says how to get the other element type


def test_default_library_is_bf16():
    out = _child(_PROBE, None)
    assert re.search(r"^path .*libpso_amd\.so$", out, flags=re.M), out
    assert "elem 1\n" in out and "compute torch.bfloat16\n" in out and "f32 0\n" in out, out
    assert "code torch.bfloat16 1\n" in out, out
    m = re.search(r"^raises torch.float16 (.*)$", out, flags=re.M)
    assert m and "PSO_LIB=f16" in m.group(1), out


def test_loss_scaler_matches_torch_grad_scaler():
    """amp.LossScaler against torch.amp.GradScaler("cpu") with growth interval 3 over the overflow pattern
    0,0,1,0,0,0,1,1,0,0,0,0: the same scale after every step; steps 3, 7 and 8 are the skipped ones."""
    import torch
    from pairwise_sample_optimization_amd.amp import LossScaler
    pattern = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    want = [65536, 65536, 32768, 32768, 32768, 65536, 32768, 16384, 16384, 16384, 32768, 32768]
    mine = LossScaler(growth_interval=3)
    ref = torch.amp.GradScaler("cpu", growth_interval=3)
    assert mine.scale == ref.get_scale() == 65536.0
    assert (mine.growth_factor, mine.backoff_factor) == (ref.get_growth_factor(), ref.get_backoff_factor())
    assert LossScaler().growth_interval == torch.amp.GradScaler("cpu").get_growth_interval() == 2000
    p = torch.nn.Parameter(torch.ones(4))
    opt = torch.optim.SGD([p], lr=0.125)
    got_mine, got_ref, skipped_mine, skipped_ref = [], [], [], []
    for i, inf in enumerate(pattern, 1):
        opt.zero_grad()
        loss = (p * (float("inf") if inf else 1.0)).sum()
        ref.scale(loss).backward()  # scale() once per iteration creates the scaler's state
        before = p.detach().clone()
        ref.step(opt)
        ref.update()
        if torch.equal(before, p.detach()):
            skipped_ref.append(i)
        got_ref.append(ref.get_scale())
        n0 = mine.skipped
        got_mine.append(mine.update(bool(inf)))
        if mine.skipped != n0:
            skipped_mine.append(i)
    assert got_ref == want, got_ref
    assert got_mine == want, got_mine
    assert skipped_mine == skipped_ref == [3, 7, 8]
    sd = mine.state_dict()
    other = LossScaler()
    other.load_state_dict(sd)
    assert other.state_dict() == sd


@pytest.mark.gpu
def test_loss_scale_needs_the_f16_library(cuda):
    """In this (bf16-library) process a trainer asked to scale its loss raises: bf16 has fp32's exponent range, and a
    scaler there would only add its per-step synchronisation."""
    from types import SimpleNamespace
    import torch
    from pairwise_sample_optimization_amd import compute_dtype
    from pairwise_sample_optimization_amd.amp import LossScaler
    from pairwise_sample_optimization_amd.trainer import PSOTrainer
    from pairwise_sample_optimization_amd.unet import UNet2DConditionModel, UNetConfig
    assert compute_dtype() == torch.bfloat16
    with torch.device(cuda):
        unet = UNet2DConditionModel(UNetConfig.tiny(16))
    unet.init_weights(0)
    unet.add_adapter(SimpleNamespace(r=8, lora_alpha=8))
    unet.prepare()
    for ls in (1024.0, LossScaler()):
        with pytest.raises(ValueError, match="PSO_LIB=f16"):
            PSOTrainer(unet, mode="turbo", num_steps=2, loss_scale=ls)
    tr = PSOTrainer(unet, mode="turbo", num_steps=2)
    assert tr.scaler is None and tr.loss_scale == 1.0


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_f16_library_on_gpu(cuda, capsys):
    """tests/test_gpu_f16.py and tests/test_gpu_loss_kernels.py in one fresh child process on libpso_amd_f16.so
    (PSO_LIB=f16): -x, so a fault ends the child at once; the child's whole log is written to
    $PSO_TEST_LOG_DIR/f16_child.log when that variable names a directory (the failure message carries its tail
    either way)."""
    assert os.path.exists(F16_LIB), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "--timeout", "300",
           "--timeout-method", "thread", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_f16.py"),
           os.path.join(ROOT, "tests", "test_gpu_loss_kernels.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=840)
    tail = r.stdout[-6000:] + r.stderr[-2000:]
    with capsys.disabled():  # the child's summary line belongs in the suite log
        print("\n[f16 child] " + (r.stdout.strip().splitlines() or ["(no output)"])[-1], flush=True)
    out_dir = os.environ.get("PSO_TEST_LOG_DIR", "")
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "f16_child.log"), "w") as f:
            f.write(r.stdout + r.stderr)
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail
