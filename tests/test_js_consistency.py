"""Cutoff consistency term of the span model, the parts that need no GPU: the two C-ABI symbols, the soundness of the float64
restatement the GPU tests compare against (js_cases.py), and the documented Python signatures."""
import ctypes
import inspect

import pytest
import torch

import js_cases as J


def test_symbols_are_bound_and_exported():
    from mtvaf_amd import hip
    from mtvaf_amd.build import build_library
    lib = ctypes.CDLL(build_library(verbose=False))
    for name in ("mtvaf_js_consistency_fwd", "mtvaf_js_consistency_bwd"):
        assert name in hip.exported_symbols()
        assert hasattr(lib, name), f"{name} is not exported by the built library"


@pytest.mark.parametrize("case", J.CASES, ids=J.case_id)
def test_masked_restatement_with_all_ones_is_the_literal_form(case):
    B, M, C = case[:3]
    x, y = J.make_logits(*case)
    ref = J.js_ref(x, y)
    assert torch.isfinite(ref)
    got = J.js_ref_masked(x, y, torch.ones(B, M, dtype=torch.long))
    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))


def test_masked_restatement_is_the_literal_form_on_compacted_sentences():
    for _, x, y, mask in J.masked_cases():
        B = x.shape[0]
        total = 0.0
        for b in range(B):
            live = mask[b] != 0
            if bool(live.any()):
                total += float(J.js_ref(x[b:b + 1, live], y[b:b + 1, live]))   # batchmean over a batch of one
        got = float(J.js_ref_masked(x, y, mask))
        assert abs(got - total / B) <= 1e-12 * max(1.0, abs(got))


def test_value_is_zero_for_one_slot_and_for_equal_logits_and_symmetric():
    x, y = J.make_logits(1, 1, 4, 1, 1)
    assert abs(float(J.js_ref(x, y))) <= 1e-15          # M = 1: both softmaxes are 1
    x, y = J.make_logits(2, 20, 4, 3, 0)
    assert torch.equal(x, y) and abs(float(J.js_ref(x, y))) <= 1e-15
    x, y = J.make_logits(5, 33, 4, 3, 1)
    a, b = float(J.js_ref(x, y)), float(J.js_ref(y, x))
    assert a > 0 and abs(a - b) <= 1e-12 * a
    _, x, y, mask = J.masked_cases()[0]
    a, b = float(J.js_ref_masked(x, y, mask)), float(J.js_ref_masked(y, x, mask))
    assert a > 0 and abs(a - b) <= 1e-12 * a


def test_reference_gradients_are_finite_on_every_case():
    for case in J.CASES:
        js, gx, gy = J.ref_with_grads(*J.make_logits(*case))
        assert torch.isfinite(js) and torch.isfinite(gx).all() and torch.isfinite(gy).all(), case
    for name, x, y, mask in J.masked_cases():
        js, gx, gy = J.ref_with_grads(x, y, mask)
        assert torch.isfinite(js) and torch.isfinite(gx).all() and torch.isfinite(gy).all(), name
        dead = (mask == 0)[:, :, None].expand_as(gx)
        assert not bool(gx[dead].any()) and not bool(gy[dead].any())


def test_python_surface_has_the_documented_signatures():
    from mtvaf_amd import engine
    from mtvaf_amd.models.bert_model import TVNetSAModel
    fwd = inspect.signature(engine.JSConsistencyFunction.forward)
    assert list(fwd.parameters) == ["ctx", "logits", "cutoff_logits", "mask", "scale"]
    assert fwd.parameters["mask"].default is None and fwd.parameters["scale"].default == 1.0
    plain = inspect.signature(TVNetSAModel.forward).parameters
    both = inspect.signature(TVNetSAModel.forward_with_cutoff).parameters
    assert list(both) == [n for n in plain if n != "augument"] + ["return_parts"]
    assert both["return_parts"].default is False
    for n in both:
        if n not in ("self", "return_parts"):
            assert both[n].default == plain[n].default, n
