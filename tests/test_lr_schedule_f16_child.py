"""The learning-rate schedule's loss-scaler cases on the fp16 library: tests/test_gpu_lr_schedule_f16.py in one fresh
PSO_LIB=f16 child process (the element type is per process), as tests/test_f16_amp_child.py runs the device scaler's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_LIB = os.path.join(ROOT, "pairwise_sample_optimization_amd", "libpso_amd_f16.so")


@pytest.mark.gpu
@pytest.mark.timeout(420)
def test_lr_schedule_cases_on_the_f16_library(cuda, capsys):
    """-x, so a fault ends the child at once; the child's whole log goes to $PSO_TEST_LOG_DIR/lr_schedule_f16_child.log
    when that variable names a directory (the failure message carries its tail either way)."""
    assert os.path.exists(F16_LIB), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "--timeout", "180",
           "--timeout-method", "thread", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_lr_schedule_f16.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=360)
    tail = r.stdout[-6000:] + r.stderr[-2000:]
    with capsys.disabled():  # the child's summary line belongs in the suite log
        print("\n[lr schedule f16 child] " + (r.stdout.strip().splitlines() or ["(no output)"])[-1], flush=True)
    out_dir = os.environ.get("PSO_TEST_LOG_DIR", "")
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "lr_schedule_f16_child.log"), "w") as f:
            f.write(r.stdout + r.stderr)
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " error" not in r.stdout, tail
    # the sync-debug case may skip itself (a torch build that does not honour the mode); nothing else may
    m = re.search(r"(\d+) skipped", r.stdout)
    assert m is None or int(m.group(1)) <= 2, tail  # its two parametrisations
