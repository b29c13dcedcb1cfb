"""Digests of the AdamW / 8-bit AdamW host-argument forms: three steps of each on inputs that are a closed-form integer
expression of the element index (no RNG), sha256 of the raw bytes of every output tensor after each step.
tests/test_gpu_optim_bits.py compares record() with tests/golden/optim_step_bits.json, which this file wrote on the
commit the JSON names; only call spellings that predate the one-entry-per-optimizer change are used here.
usage (GPU): python tools/optim_bits.py --commit $(git rev-parse HEAD) --out tests/golden/optim_step_bits.json"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pairwise_sample_optimization_amd import kernels as K  # noqa: E402

STEPS = 3
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
GRAD_SCALE = 0.5
CLIP = (1.5, 0.625)  # (norm, coefficient) as pso_grad_clip_coef leaves them; the step reads the coefficient
N_FLAT = 4101  # fp32 AdamW and the uniform 8-bit form: two full blocks and a 5-element (scalar-tail) block
# (offset, numel) inside one flat buffer, every offset 16-B aligned, a gap after each tensor: 3000 -> 32-bit state, two
# blocks, the second ragged; 4096 -> two full 8-bit blocks; 4101 -> a 5-element last block; 2050 -> 32-bit state with
# a 2-element block
SEGMENTS = [(0, 3000), (3004, 4096), (7104, 4101), (11208, 2050)]
N_SEG = 13260


def _unit(n, salt):
    """[-1, 1) from the element index: ((i * 1103515245 + 12345 + 7919 * salt) mod 65521) / 65521 * 2 - 1, the integer
    part in int64 (exact), the rest in fp64."""
    i = torch.arange(n, dtype=torch.int64)
    return ((i * 1103515245 + 12345 + 7919 * salt) % 65521).double() / 65521.0 * 2.0 - 1.0


def _param(n, dev):
    return (_unit(n, 0) * 2e-2).float().to(dev)


def _grad(n, step, bad, dev):
    """The step's gradient (about 1e-2); step 2 carries one inf and one nan element at the two indices of `bad`."""
    g = (_unit(n, step) * 1e-2).float()
    if step == 2:
        g[bad[0]] = float("inf")
        g[bad[1]] = float("nan")
    return g.to(dev)


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _adamw(dev, clip):
    p = _param(N_FLAT, dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = {}
    for step in range(1, STEPS + 1):
        g = _grad(N_FLAT, step, (10, 4099), dev)
        K.adamw_step(p, g, m, v, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], step,
                     grad_scale=GRAD_SCALE, clip=clip)
        out[f"step{step}"] = {"param": _digest(p), "exp_avg": _digest(m), "exp_avg_sq": _digest(v)}
    return out


def _adamw8bit(dev, clip, n, segments, bad):
    p = _param(n, dev)
    pw = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    state = K.Adam8State(n, dev, segments=segments)
    out = {}
    for step in range(1, STEPS + 1):
        g = _grad(n, step, bad, dev)
        K.adamw8bit_step(p, g, state, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], step,
                         grad_scale=GRAD_SCALE, clip=clip, out_bf16=pw,
                         zero_grad=segments is not None and step % 2 == 1)
        d = {name: _digest(t) for name, t in state.tensors().items() if name != "block_table"}
        d.update(param=_digest(p), param_bf16=_digest(pw), grad=_digest(g))
        out[f"step{step}"] = d
    return out


def record(dev):
    """{form: {"step1".."step3": {tensor name: sha256 hex}}} of the four host forms."""
    clip = torch.tensor(CLIP, dtype=torch.float32, device=dev)
    # inf in the first 8-bit tensor, nan in the first 32-bit one
    seg_bad = (SEGMENTS[1][0] + 5, SEGMENTS[0][0] + 7)
    out = {"adamw": _adamw(dev, None), "adamw_clip": _adamw(dev, clip),
           "adamw8bit_uniform_bf16": _adamw8bit(dev, clip, N_FLAT, None, (10, 4099)),
           "adamw8bit_blocks_zero_grad": _adamw8bit(dev, clip, N_SEG, SEGMENTS, seg_bad)}
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the libraries were built from")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    doc = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "digests": record(torch.device("cuda", 0))}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["digests"], sort_keys=True))


if __name__ == "__main__":
    main()
