"""Child process of tests/test_gpu_lora_merge_f16.py (PSO_LIB=f16: the element type is per process): the kernel bound
cases of tests/test_gpu_lora_merge.py and its plain-LoRA UNet case (tiny16, r = 8) on the fp16 library, at the same
bound (with fp16's ulp) and the same bar."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lora_merge_ref as R
    from pairwise_sample_optimization_amd import _lib
    assert _lib.F16 and _lib.ELEM_DTYPE == torch.float16
    cuda = torch.device("cuda:0")
    R.kernel_bound_cases(cuda)
    c = R.gpu_plain_case(8, cuda)
    assert c.unet.lora.work.dtype == torch.float16 and c.unet._merged.kv[128].dtype == torch.float16
    assert c.moved >= 3 * R.FWD_BAR, c.moved
    assert c.fused_err < R.FWD_BAR, (c.fused_err, c.adapter_err)
    print(f"LORA_MERGE_F16_OK moved={c.moved:.3e} adapter={c.adapter_err:.3e} fused={c.fused_err:.3e}", flush=True)


if __name__ == "__main__":
    main()
