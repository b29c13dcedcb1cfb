"""The host-argument forms of pso_adamw_step / pso_adamw8bit_step return the bits recorded at the commit that
tests/golden/optim_step_bits.json names (tools/optim_bits.py, run on the MI355X before the two optimizers were given
one entry each): fp32 AdamW with and without the clip coefficient, the uniform 8-bit form with the bf16 working copy,
and the block-table form with zero_grad on odd steps -- three steps each, step 2 with one inf and one nan gradient
element.  The amp_state and lr_dev forms are pinned onto these bit for bit by test_gpu_amp_device.py and
test_gpu_lr_schedule.py."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_step_bits.json")


def test_host_form_steps_return_the_recorded_bits(cuda):
    from tools import optim_bits
    want = json.load(open(GOLDEN))
    got = optim_bits.record(cuda)
    assert got.keys() == want["digests"].keys()
    bad = []
    for form, steps in want["digests"].items():
        assert got[form].keys() == steps.keys(), form
        for step, tensors in steps.items():
            assert got[form][step].keys() == tensors.keys(), (form, step)
            bad += [f"{form} {step} {name}" for name, dig in tensors.items() if got[form][step][name] != dig]
    assert not bad, f"bits differ from commit {want['commit'][:12]} in: " + "; ".join(bad)
