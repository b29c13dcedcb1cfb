"""Merged-weight LoRA inference on the fp16 library: the element type is per process, so the cases run in a fresh
child (tests/lora_merge_f16_worker_gpu.py), the way tests/dora_f16_worker_gpu.py is run."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_lora_merge_on_the_f16_library(cuda):
    lib = os.path.join(ROOT, "pairwise_sample_optimization_amd", "libpso_amd_f16.so")
    assert os.path.exists(lib), "libpso_amd_f16.so not built (make -C pairwise_sample_optimization_amd/csrc)"
    env = dict(os.environ, PSO_LIB="f16")
    env.pop("PSO_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "lora_merge_f16_worker_gpu.py")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    tail = r.stdout[-4000:] + r.stderr[-4000:]
    print(tail)
    assert r.returncode == 0, tail
    assert "LORA_MERGE_F16_OK" in r.stdout, tail
