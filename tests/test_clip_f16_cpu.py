"""CPU checks of the f16 opt-in of the CLIP towers (clip.py `allow_f16`) and of the image-kind entry
pso_clip_preprocess_img.  The element type is per process, so each library gets a fresh child process (PSO_LIB=f16 /
knobs / unset), the way tests/test_abi.py probes the three builds; nothing here needs a GPU."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MODELS = """
import json
import torch
from pairwise_sample_optimization_amd import _lib
from pairwise_sample_optimization_amd.clip import (CLIPModel, CLIPTextConfig, CLIPTextModel,
                                                   CLIPTextModelWithProjection, CLIPTextTransformer,
                                                   CLIPVisionConfig, CLIPVisionTransformer)
tc = CLIPTextConfig(vocab_size=100, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                    projection_dim=16)
vc = CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28,
                      patch_size=14, projection_dim=16)
builders = {"text": lambda **kw: CLIPTextModel(tc, **kw),
            "text_proj": lambda **kw: CLIPTextModelWithProjection(tc, **kw),
            "clip": lambda **kw: CLIPModel(tc, vc, 16, **kw), "text_tower": lambda **kw: CLIPTextTransformer(tc, **kw),
            "vision_tower": lambda **kw: CLIPVisionTransformer(vc, **kw)}
report = {"elem": str(_lib.ELEM_DTYPE), "f16": _lib.F16, "refused": {}, "keys": {}, "dtypes": {}, "loaded": {}}
for name, build in builders.items():
    try:
        build()
        report["refused"][name] = None
    except _lib.PsoLibError as e:
        report["refused"][name] = str(e)
    for dev in ("meta", "cpu"):
        with torch.device(dev):
            m = build(allow_f16=True)
        report["dtypes"][name + ":" + dev] = sorted({str(v.dtype) for k, v in m.state_dict().items()
                                                     if k != "logit_scale"})
    report["keys"][name] = sorted(m.state_dict())
    if name in ("text", "text_proj", "clip"):
        # a checkpoint as it comes from disk: fp32 tensors, and the position_ids buffer old checkpoints carry
        g = torch.Generator().manual_seed(0)
        sd = {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items()}
        sd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
        m.load_state_dict(sd)
        got = m.state_dict()
        report["loaded"][name] = {
            "dtypes": sorted({str(v.dtype) for k, v in got.items() if k != "logit_scale"}),
            "logit_scale": str(got["logit_scale"].dtype) if "logit_scale" in got else None,
            "values": all(torch.equal(got[k], sd[k].to(got[k].dtype)) for k in got)}
# every from_config / from_pretrained hands the keyword on (from_pretrained calls from_config)
with torch.device("meta"):
    d = {"hidden_size": 32, "intermediate_size": 64, "num_hidden_layers": 1, "num_attention_heads": 2, "vocab_size": 50}
    CLIPTextModel.from_config(d, allow_f16=True)
    CLIPTextModelWithProjection.from_config(d, allow_f16=True)
    m = CLIPModel.from_config({"projection_dim": 16, "text_config": d, "vision_config": dict(d, image_size=28)},
                              allow_f16=True)
    report["from_config_flag"] = m.allow_f16
    refused = 0
    for call in (lambda: CLIPTextModel.from_config(d), lambda: CLIPTextModelWithProjection.from_config(d),
                 lambda: CLIPModel.from_config({"projection_dim": 16, "text_config": d, "vision_config": d})):
        try:
            call()
        except _lib.PsoLibError:
            refused += 1
    report["from_config_refused"] = refused
print("REPORT " + json.dumps(report))
"""

_ENTRY = """
import ctypes
import torch
from pairwise_sample_optimization_amd import _lib
l = _lib.lib()
print("ARITY", len(_lib.SIGNATURES["pso_clip_preprocess_img"][1]), len(_lib.SIGNATURES["pso_clip_preprocess"][1]))
print("BOUND", l.pso_clip_preprocess_img.argtypes == _lib.SIGNATURES["pso_clip_preprocess_img"][1])
print("KINDS", _lib.IMG_F32, _lib.IMG_ELEM, _lib.IMG_U8)
if not torch.cuda.is_available():
    # fake addresses, never dereferenced: every call fails an argument check before any launch (host-only on purpose,
    # as in tests/test_abi.py: with a GPU present a regression would launch on them)
    P = 0x10000
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    need = l.pso_clip_preprocess_ws_bytes(1, 32, 32, 28)
    for name, kind, size, kpad, ws in (("kind3", 3, 28, 592, need), ("kind-1", -1, 28, 592, need),
                                       ("size", _lib.IMG_ELEM, 30, 592, need), ("kpad", _lib.IMG_U8, 28, 580, need),
                                       ("ws", _lib.IMG_F32, 28, 592, need - 1)):
        rc = l.pso_clip_preprocess_img(1, 32, 32, P, kind, size, 14, kpad, m, m, 2 * P, 3 * P, ws, None)
        print("case", name, rc, l.pso_last_error().decode())
"""


def _child(pso_lib, script):
    env = {k: v for k, v in os.environ.items() if k not in ("PSO_LIB", "PSO_LIB_PATH")}
    if pso_lib:
        env["PSO_LIB"] = pso_lib
    r = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (pso_lib, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def _report(pso_lib):
    out = _child(pso_lib, _MODELS)
    return json.loads(re.search(r"^REPORT (.*)$", out, flags=re.M).group(1))


def test_f16_library_refuses_by_default_and_builds_with_the_keyword():
    f16, bf16 = _report("f16"), _report(None)
    assert f16["f16"] and f16["elem"] == "torch.float16"
    assert not bf16["f16"] and bf16["elem"] == "torch.bfloat16"
    # the default constructors keep raising under f16, with the text the pinned refusal test matches
    for name, msg in f16["refused"].items():
        assert msg is not None and "f16 library" in msg and "allow_f16=True" in msg, (name, msg)
    assert f16["from_config_refused"] == 3 and f16["from_config_flag"] is True
    # with the keyword they build on meta and on cpu, in fp16
    for key, dts in f16["dtypes"].items():
        assert dts == ["torch.float16"], (key, dts)
    # load_state_dict of fp32 tensors: fp16 parameters with the RNE-rounded values, fp32 logit_scale
    for name, got in f16["loaded"].items():
        assert got["dtypes"] == ["torch.float16"] and got["values"], (name, got)
    assert f16["loaded"]["clip"]["logit_scale"] == "torch.float32"
    # the same keys as the bf16 models: one checkpoint layout for both libraries
    assert f16["keys"] == bf16["keys"]
    assert any(k.startswith("vision_model.") for k in f16["keys"]["clip"]) and "logit_scale" in f16["keys"]["clip"]
    # under the bf16 library nothing is refused, the keyword is accepted and ignored: bf16 parameters
    assert all(msg is None for msg in bf16["refused"].values()) and bf16["from_config_refused"] == 0
    for key, dts in bf16["dtypes"].items():
        assert dts == ["torch.bfloat16"], (key, dts)
    for name, got in bf16["loaded"].items():
        assert got["dtypes"] == ["torch.bfloat16"] and got["values"], (name, got)
    assert bf16["loaded"]["clip"]["logit_scale"] == "torch.float32"


def _header_arity(name):
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"\b%s\(([^)]*)\);" % name, h)
    assert m, name + " is not declared in include/pso_amd.h"
    return len(m.group(1).split(","))


def test_preprocess_img_entry_is_bound_in_all_three_libraries():
    h = open(os.path.join(ROOT, "include", "pso_amd.h")).read()
    kinds = {k: int(v) for k, v in re.findall(r"^#define (PSO_IMG_\w+) (\d+)", h, flags=re.M)}
    assert kinds == {"PSO_IMG_F32": 0, "PSO_IMG_ELEM": 1, "PSO_IMG_U8": 2}
    n = _header_arity("pso_clip_preprocess_img")
    assert n == _header_arity("pso_clip_preprocess") == 14
    for pso_lib in (None, "knobs", "f16"):
        out = _child(pso_lib, _ENTRY)
        assert f"ARITY {n} {n}" in out and "BOUND True" in out and "KINDS 0 1 2" in out, (pso_lib, out)
        got = {m.group(1): (int(m.group(2)), m.group(3))
               for m in re.finditer(r"^case (\S+) (-?\d+) (.*)$", out, flags=re.M)}
        if not got:  # a GPU is present: the argument probes are host-only
            continue
        assert sorted(got) == ["kind-1", "kind3", "kpad", "size", "ws"], (pso_lib, out)
        for name, (rc, msg) in got.items():
            assert rc == 1 and msg.startswith("pso_clip_preprocess_img: "), (pso_lib, name, rc, msg)  # PSO_ERR_ARG
        assert "img_kind" in got["kind3"][1] and "img_kind" in got["kind-1"][1]
        assert ("fp16" if pso_lib == "f16" else "bf16") in got["kind3"][1]
        assert "workspace too small" in got["ws"][1]
