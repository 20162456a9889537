"""Candidate-span proposal, the parts that need no GPU: the restatement of the rule (tests/span_propose_cases.py) against the lists
the reference's span_annotate_candidates returned (tests/golden/span_candidates_ref.npz), the C entry point's argument checks,
the binding and the host helpers of mtvaf_amd.spans."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import span_propose_cases as C

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "span_candidates_ref.npz")


def golden_cases():
    fx = np.load(GOLDEN)
    for c in range(int(fx["n_cases"])):
        n_best, max_len, heur, use_nms, em = (int(x) for x in fx[f"c{c}_scalars"])
        yield dict(c=c, sl=fx[f"c{c}_start_logits"], el=fx[f"c{c}_end_logits"], wi=fx[f"c{c}_word_index"], wk=fx[f"c{c}_word_key"],
                   n_best=n_best, max_len=max_len, heur=heur, nms=int(bool(use_nms) and not em), thr=float(fx[f"c{c}_threshold"]),
                   span_starts=fx[f"c{c}_span_starts"], span_ends=fx[f"c{c}_span_ends"], label_masks=fx[f"c{c}_label_masks"],
                   labels=fx[f"c{c}_labels"])


def test_restatement_equals_the_reference_lists():
    n = 0
    for g in golden_cases():
        got = C.propose(g["sl"], g["el"], g["wi"], g["wk"], g["n_best"], g["max_len"], g["thr"], g["heur"], g["nms"])
        for k in ("span_starts", "span_ends", "label_masks"):
            assert np.array_equal(got[k], g[k]), (g["c"], k, got[k], g[k])
        assert not g["labels"].any()
        assert np.array_equal(got["count"], g["label_masks"].sum(1))
        n += int(got["count"].sum())
    assert n > 50  # the fixture accepts spans, with and without nms


def test_restatement_edge_rows():
    """The rows the case table promises: all-filtered, fewer survivors than n_best / 2, a padded position holding the maximum."""
    sl, el, wi, wk = C.make_inputs(3, 70, seed=1)
    out = C.propose(sl, el, wi, wk, 20, 12, C.THRESHOLD, 1, 0)
    assert out["count"][1] == 0 and not any(out[k][1].any() for k in ("span_starts", "span_ends", "label_masks", "span_scores"))
    assert 1 <= out["count"][2] < 10
    assert out["count"][0] > 0 and (out["span_ends"][0] < 69).all() and (out["span_starts"][0][:out["count"][0]] > 0).all()
    sl, el, wi, _ = C.make_inputs(70, 9, seed=2)
    odd = C.propose(sl, el, wi, None, 5, 12, -100.0, 0, 0)
    assert odd["count"].max() == 3 and (odd["count"] == 3).sum() > 5  # an odd n_best accepts ceil(n_best / 2)


def test_symbol_exported_and_bound():
    from mtvaf_amd import hip
    from mtvaf_amd.build import build_library
    assert "mtvaf_span_propose" in hip.exported_symbols()
    lib = ctypes.CDLL(build_library(verbose=False))
    assert hasattr(lib, "mtvaf_span_propose")
    assert hip.lib().mtvaf_span_propose.argtypes == hip._SIGS["mtvaf_span_propose"][1] == abi_header.signature("mtvaf_span_propose")[1]


@pytest.mark.parametrize("S,n_best", [(0, 20), (513, 20), (16, 0), (16, 33)])
def test_limits_are_checked_before_any_launch(S, n_best):
    """The library answers its shape status without touching the device; the Python layer raises ValueError."""
    from mtvaf_amd import hip
    rc = hip.lib().mtvaf_span_propose(None, 2, None, None, None, None, None, None, None, 2, S, n_best, 12, 8.0, 1, 0, None)
    assert rc == -1
    with pytest.raises(ValueError):
        hip.span_propose(torch.zeros(2, S, 2), torch.zeros(2, S, dtype=torch.int32), n_best=n_best)


def test_bad_nms_and_shapes_raise():
    from mtvaf_amd import hip
    with pytest.raises(ValueError):
        hip.span_propose(torch.zeros(2, 8, 2), torch.zeros(2, 8, dtype=torch.int32), nms=2)
    with pytest.raises(ValueError):
        hip.span_propose(torch.zeros(2, 8, 2), torch.zeros(2, 9, dtype=torch.int32))
    with pytest.raises(ValueError):
        hip.span_propose(torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32))


def test_word_keys_and_token_maps():
    from mtvaf_amd import spans
    ids, vocab = spans.word_keys([["The", "screen", "the", "Screen"], ["battery", "screen"]])
    assert ids == [[0, 1, 0, 1], [2, 1]] and vocab == {"the": 0, "screen": 1, "battery": 2}
    more, vocab2 = spans.word_keys([["Battery", "life"]], vocab)
    assert more == [[2, 3]] and vocab2 is vocab
    t2w = spans.batch_token_to_word([{1: 0, 2: 1, 3: 1, 4: 2, 5: 3}, {1: 0, 2: 1}], 8)
    assert t2w.dtype == torch.int32
    assert t2w.tolist() == [[-1, 0, 1, 1, 2, 3, -1, -1], [-1, 0, 1, -1, -1, -1, -1, -1]]
    keys = spans.token_word_keys(t2w, ids)
    assert keys.tolist() == [[-1, 0, 1, 1, 0, 1, -1, -1], [-1, 2, 1, -1, -1, -1, -1, -1]]
    with pytest.raises(ValueError):
        spans.token_to_word({9: 0}, 8)
