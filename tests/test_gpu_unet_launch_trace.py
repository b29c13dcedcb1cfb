"""The UNet issues the same kernel-wrapper calls, in the same order, with the same operand shapes, as the commit the
fixture was recorded on.

unet.py decides per adapted projection (qkv, o1, q2, kv2, o2) which of seven forms runs (unet.proj_form) and spends
the rest of BasicTransformerBlock.fwd / bwd issuing launches through `kernels`.  A recorder wraps every public
function of `kernels` (through the module object, so unet's `K.gemm(...)` sees it) and TnRankQueue.add / flush for
one forward_nhwc (+ backward_nhwc) and notes, per call, the name, the shape and dtype of every tensor argument and
every scalar argument -- bound to the wrapper's signature with its defaults filled in, so that spelling out a default
or passing an argument by keyword is no difference, and any other operand is.  tests/golden/unet_launch_trace.json
holds, per mode of tools/unet_digest.MODES, the call count, a per-name count (so that a mismatch says where) and the
sha256 of the canonical sequence.

What this sees and what it does not: a missing, added or reordered launch, another shape, dtype or scalar argument.
It notes no addresses, so an operand swapped for another of the same shape and dtype -- the merged weight for the
base weight (`fused` and `adapters_off` share one digest), o1 for o2, a wrong e4m3 cache key -- passes here; rank 4
runs padded to 8, so `paired_r4` and `paired_r8` share one too.  Those are for the bit digests of
tools/unet_digest.py (run by hand on two commits) and the parity tests.

The fixture was recorded by `python tests/test_gpu_unet_launch_trace.py --record` on commit 78d6f43 ("EMA of the
trained weights for both trainers"), the parent of the change that moved the five projection ladders into
unet._proj_fwd / _proj_bwd -- never on the code under test.  Re-record it only on a commit whose launch sequence is
meant to be the new truth, and say so in that commit."""
import hashlib
import inspect
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "unet_launch_trace.json")

pytestmark = pytest.mark.gpu


def _desc(v):
    if isinstance(v, torch.Tensor):
        return ["T", list(v.shape), str(v.dtype)]
    if isinstance(v, (tuple, list)):
        return [_desc(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__  # callables, devices: the kind only


class Recorder:
    """with Recorder() as rec: ... -> rec.calls = [[name, {parameter: value}]] in issue order."""

    def __enter__(self):
        from pairwise_sample_optimization_amd import kernels as K
        self.calls, self._undo = [], []

        def wrap(owner, attr, name):
            fn = getattr(owner, attr)
            sig = inspect.signature(fn)

            def rec(*a, **kw):
                ba = sig.bind(*a, **kw)
                ba.apply_defaults()
                self.calls.append([name, {k: _desc(v) for k, v in ba.arguments.items() if k != "self"}])
                return fn(*a, **kw)
            setattr(owner, attr, rec)
            self._undo.append((owner, attr, fn))

        for attr, fn in sorted(vars(K).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == K.__name__ and not attr.startswith("_"):
                wrap(K, attr, attr)
        wrap(K.TnRankQueue, "add", "TnRankQueue.add")
        wrap(K.TnRankQueue, "flush", "TnRankQueue.flush")
        return self

    def __exit__(self, *exc):
        for owner, attr, fn in self._undo:
            setattr(owner, attr, fn)

    def summary(self):
        by_name = {}
        for c in self.calls:
            by_name[c[0]] = by_name.get(c[0], 0) + 1
        canon = json.dumps(self.calls, sort_keys=True, separators=(",", ":"))
        return {"calls": len(self.calls), "by_name": dict(sorted(by_name.items())),
                "sha256": hashlib.sha256(canon.encode()).hexdigest()}


def trace(name, dev):
    from tools import unet_digest as D
    unet, inp = D.build(name, dev)
    with Recorder() as rec:
        D.run(name, unet, inp)
    torch.cuda.synchronize()
    return rec.summary()


def _modes():
    from tools.unet_digest import MODES
    return list(MODES)


@pytest.mark.parametrize("mode", _modes())
def test_launch_sequence_is_the_recorded_one(cuda, mode):
    with open(FIXTURE) as f:
        want = json.load(f)[mode]
    got = trace(mode, cuda)
    diff = {k: (want["by_name"].get(k, 0), got["by_name"].get(k, 0))
            for k in sorted(set(want["by_name"]) | set(got["by_name"]))
            if want["by_name"].get(k, 0) != got["by_name"].get(k, 0)}
    print(f"{mode}: {got['calls']} calls (recorded {want['calls']}), sha256 {got['sha256']}")
    assert not diff, f"{mode}: calls per function (recorded, now): {diff}"
    assert got["calls"] == want["calls"]
    assert got["sha256"] == want["sha256"], f"{mode}: same counts, other order or operands"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_gpu_unet_launch_trace.py --record"
    out = {m: trace(m, torch.device("cuda:0")) for m in _modes()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} modes -> {FIXTURE}")
