"""The EMA under fp16 training with a device-resident loss scaler: the element type is per process, so the case runs in
a fresh child (tests/ema_f16_worker_gpu.py), the way tests/prodigy_f16_worker_gpu.py is run."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_ema_counts_skipped_steps_under_the_device_scaler(cuda):
    lib = os.path.join(ROOT, "pairwise_sample_optimization_amd", "libpso_amd_f16.so")
    assert os.path.exists(lib), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "ema_f16_worker_gpu.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    tail = r.stdout[-4000:] + r.stderr[-4000:]
    print(tail)
    assert r.returncode == 0, tail
    assert "EMA_F16_OK" in r.stdout, tail
