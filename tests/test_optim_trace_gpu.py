"""The launches of `mtvaf_amd.optim.AdamW`, call by call, against the trace recorded in tests/golden/adamw_launch_trace.json
(optim_trace.py: what is recorded, and the scenarios; `python tools/adamw_trace.py --write` regenerates the file).  The wrappers of
`mtvaf_amd.hip` turn equal arguments into equal kernel arguments, so an equal trace is an optimizer that computes the same bits."""
import json

import pytest

import optim_trace as T

pytestmark = pytest.mark.gpu

with open(T.GOLDEN) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def scenarios():
    return T.scenarios()


@pytest.mark.parametrize("key", list(WANT))
def test_scenario_issues_the_recorded_calls_with_the_recorded_arguments_in_the_recorded_order(key, scenarios):
    got = json.loads(json.dumps(scenarios[key]()))
    assert [c[0] for c in got] == [c[0] for c in WANT[key]]
    for i, (a, b) in enumerate(zip(got, WANT[key])):
        assert a == b, (i, a, b)


def test_the_record_holds_every_scenario_and_every_form_of_the_update(scenarios):
    assert list(scenarios) == list(WANT)
    names = {c[0] for calls in WANT.values() for c in calls}
    forms = {f"adamw{p}{s}{d}" for p in ("", "_planes") for s in ("", "_seg") for d in ("", "_sched")}
    assert forms | {"adamw_multi", "adamw_multi_sched", "adamw_sched_advance", "grad_sqnorm", "grad_clip_finalize", "swap_f32",
                    "sam_finalize", "sam_perturb", "sam_perturb_planes", "sam_perturb_multi", "sam_restore", "sam_restore_planes",
                    "sam_restore_multi", "planes_for_update", "shadow_for_update", "planes_written", "shadow_written", "planes_rewrite",
                    "invalidate_weight_images"} <= names, sorted(names)
