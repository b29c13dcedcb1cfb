"""The CLIP towers, the PickScore reward and one whole online PSO epoch on the fp16 library (allow_f16=True): the
element type is per process, so the cases run in one fresh child (tests/clip_f16_worker_gpu.py), the way
tests/ema_f16_worker_gpu.py is run.  The child ends at its first failure; its figures are printed either way."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(420)
def test_clip_towers_pickscore_and_one_epoch_on_the_f16_library(cuda):
    lib = os.path.join(ROOT, "pairwise_sample_optimization_amd", "libpso_amd_f16.so")
    assert os.path.exists(lib), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "clip_f16_worker_gpu.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=360)
    tail = r.stdout[-6000:] + r.stderr[-4000:]
    print(tail)
    assert r.returncode == 0, tail
    assert "CLIP_F16_OK" in r.stdout, tail
