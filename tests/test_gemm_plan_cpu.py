"""The GEMM dispatch (csrc/gemm_plan.h) against the recorded table tests/golden/gemm_dispatch_table.json.

The table holds, for every case of tests/gemm_plan_cases.py, the kernel form the commit named in it launched through
the real entry points (recorded from the kernel names the entries note before launching, on a machine without a
device).  Every case must get the same plan from pso_gemm_plan_query, which launches nothing: a changed threshold
shows here as the list of shapes that moved.  Runs in a PSO_LIB=knobs child process (the query exists in the tools
build only)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch_table.json")

_PROBE = """
import ctypes, json, sys
sys.path.insert(0, "tests")
import gemm_plan_cases as C
from pairwise_sample_optimization_amd import _lib
l = _lib.lib()
got = []
for case in C.cases():
    q, info = _lib.PsoGemmPlanQuery(**C.full(case)), _lib.PsoGemmPlanInfo()
    kind = C.KIND[case["entry"]]
    rc = l.pso_gemm_plan_query(kind, ctypes.byref(q), ctypes.byref(info))
    got.append(C.plan_of_info(kind, info) if rc == 0 else ["error", rc, l.pso_last_error().decode()])
json.dump(got, sys.stdout)
"""

# the forms gemm_plan.h can choose from these entries: the 2-phase tile, the 8-phase 256 / 160 / 320 and conv 320
# forms, skinny and small-conv (GemmForm), and the rank-r / 256 / 128 / 64 TN kernels (TnKind)
_REACHABLE_FORMS = 7 + 4


def test_every_case_plans_what_the_table_recorded():
    import gemm_plan_cases as C
    table = json.load(open(TABLE))
    cases = C.cases()
    assert len(cases) == len(table["index"]) <= 20000
    assert table["fields"] == list(C.PLAN_FIELDS)
    assert len(table["plans"]) >= _REACHABLE_FORMS
    families = {(p[0], p[2] if p[0] == "8p" else 0, p[7] if p[0] == "8p" else 0) for p in table["plans"]}
    assert len(families) >= _REACHABLE_FORMS, sorted(families)  # a table collapsed onto few forms cannot pass
    env = {k: v for k, v in os.environ.items() if k != "PSO_LIB_PATH"}
    env["PSO_LIB"] = "knobs"
    r = subprocess.run([sys.executable, "-c", _PROBE], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout)
    assert len(got) == len(cases)
    moved = [(case, table["plans"][i], g) for case, i, g in zip(cases, table["index"], got) if table["plans"][i] != g]
    assert not moved, f"{len(moved)} of {len(cases)} cases moved (case, recorded, planned): {moved[:20]}"


def test_case_list_covers_every_variant_and_entry():
    import gemm_plan_cases as C
    import re
    cases = C.cases()
    h = open(os.path.join(ROOT, "include", "pso_amd_knobs.h")).read()
    named = {int(v) for v in re.findall(r"^\s*PSO_GV_\w+ = (\d+)", h, flags=re.M)}
    assert named - {0} == set(C.VARIANTS)  # the enum names exactly the numbers in use
    assert {c.get("variant", 0) for c in cases if c["entry"] == "pso_gemm"} == named
    assert {c["entry"] for c in cases} == set(C.KIND)
