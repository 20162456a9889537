"""Aspect scoring of the span model, the parts that need no GPU: the restatement of the rule (tests/span_score_cases.py) against the
counts the reference's eval_absa returned (tests/golden/span_score_ref.npz) and against hand-derived answers for every bullet of
the rule, `SpanScorer.compute`'s arithmetic, the wrapper's limits and the model switch."""
import os
import types

import numpy as np
import pytest
import torch

import abi_header
import span_score_cases as C
from span_propose_cases import signature

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "span_score_ref.npz")
NAMES = ("span_starts", "span_ends", "label_masks", "logits", "gold_starts", "gold_ends", "gold_class", "gold_masks", "word_index",
         "word_key")


def golden_cases():
    fx = np.load(GOLDEN)
    for c in range(int(fx["n_cases"])):
        yield c, {k: fx[f"c{c}_{k}"] for k in NAMES}, [int(x) for x in fx[f"c{c}_counts"]]


def test_restatement_equals_the_reference_counts():
    seen_partial = False
    for c, inp, (common, retrieved, relevant) in golden_cases():
        K = inp["logits"].shape[2]
        got = C.score(**inp)
        assert C.totals(got["counts"], K) == (common, retrieved, relevant), c
        assert got["counts"][3 * K + 1] == inp["logits"].shape[0]
        assert 0 < common
        seen_partial |= common < retrieved and common < relevant
    assert seen_partial and c == 5


# ---- hand-derived answers ----------------------------------------------------------------------------------------------------
#  token        0     1    2    3    4    5    6    7    8    9
#               [CLS] ba   ##x  ko   mi   ##y  ba   ##x  ko   [SEP]
WI = np.array([[-1, 0, 0, 1, 2, 2, 3, 3, 4, -1]], np.int32)
WK = np.array([[-1, 7, 7, 8, 9, 9, 7, 7, 8, -1]], np.int32)   # words 0 and 3 are the same string, so are 1 and 4
K = 4


def one_hot(classes):
    out = np.zeros((1, len(classes), K), np.float32)
    for n, c in enumerate(classes):
        out[0, n, c] = 1.0
    return out


def run(pred, gold, logits=None, word_key=WK):
    """pred: [(s, e, class, mask)], gold: [(s, e, class, mask)] of the one sentence above"""
    a = lambda rows, j: np.array([[r[j] for r in rows]], np.int64)  # noqa: E731
    return C.score(a(pred, 0), a(pred, 1), a(pred, 3), one_hot([r[2] for r in pred]) if logits is None else logits,
                   a(gold, 0), a(gold, 1), a(gold, 2), a(gold, 3), WI, word_key)


def counter(per_class=None, other=0, sentences=1):
    c = np.zeros(3 * K + 2, np.int64)
    for k, triple in (per_class or {}).items():
        c[3 * k:3 * k + 3] = triple   # retrieved, relevant, common
    c[3 * K], c[3 * K + 1] = other, sentences
    return c.tolist()


def test_a_match_needs_equal_signature_and_equal_class():
    got = run([(1, 2, 2, 1), (3, 3, 2, 1), (1, 2, 3, 1)], [(1, 2, 2, 1)])
    assert got["counts"].tolist() == counter({2: (2, 1, 1), 3: (1, 0, 0)})
    assert got["pred_class"].tolist() == [[2, 2, 3]] and got["matched_gold"].tolist() == [[0, -1, -1]]


def test_mask_zero_slots_do_not_exist():
    got = run([(1, 2, 2, 0), (3, 3, 1, 1)], [(1, 2, 2, 0), (3, 3, 1, 1), (1, 2, 2, 0)])
    assert got["counts"].tolist() == counter({1: (1, 1, 1)})
    assert got["pred_class"].tolist() == [[-1, 1]] and got["matched_gold"].tolist() == [[-1, 1]]


def test_an_invalid_predicted_slot_is_retrieved_and_never_hits():
    # [CLS], [SEP], beyond the sentence, a negative start, e < s -- against gold slots of the same (invalid) coordinates
    bad = [(0, 0), (3, 9), (3, 10), (-1, 3), (4, 3)]
    got = run([(s, e, 2, 1) for s, e in bad], [(s, e, 2, 1) for s, e in bad])
    assert got["counts"].tolist() == counter({2: (5, 5, 0)})
    assert got["matched_gold"].tolist() == [[-1] * 5]


def test_an_invalid_gold_slot_is_relevant_and_unmatchable():
    got = run([(3, 3, 1, 1)], [(0, 0, 1, 1), (3, 3, 1, 1)])  # the truncated term in front: the match is slot 1
    assert got["counts"].tolist() == counter({1: (1, 2, 1)})
    assert got["matched_gold"].tolist() == [[1]]


def test_gold_classes_outside_the_range_go_to_relevant_other():
    got = run([(3, 3, 0, 1), (1, 2, 3, 1)], [(3, 3, 4, 1), (3, 3, -1, 1), (1, 2, 3, 1)])
    assert got["counts"].tolist() == counter({0: (1, 0, 0), 3: (1, 1, 1)}, other=2)
    assert got["matched_gold"].tolist() == [[-1, 2]]
    assert C.totals(got["counts"], K) == (1, 2, 3)


def test_argmax_ties_resolve_to_the_lowest_index():
    logits = np.array([[[0.5, 2.0, 2.0, -1.0], [3.0, 3.0, 3.0, 3.0], [-2.0, -2.0, -1.0, -1.0]]], np.float32)
    got = run([(3, 3, 0, 1)] * 3, [(3, 3, 1, 1), (3, 3, 2, 1)], logits=logits)
    assert got["pred_class"].tolist() == [[1, 0, 2]]
    assert got["counts"].tolist() == counter({0: (1, 0, 0), 1: (1, 1, 1), 2: (1, 1, 1)})
    assert got["matched_gold"].tolist() == [[0, -1, 1]]


def test_duplicate_gold_and_duplicate_predictions():
    # "ba" stands at words 0 and 3: two gold terms of equal text count twice and let one prediction hit once, on the lower slot
    got = run([(1, 2, 2, 1)], [(6, 7, 2, 1), (1, 2, 2, 1)])
    assert got["counts"].tolist() == counter({2: (1, 2, 1)}) and got["matched_gold"].tolist() == [[0]]
    # two predictions of equal signature each count and each hit
    got = run([(1, 2, 2, 1), (6, 7, 2, 1), (1, 2, 2, 1)], [(6, 7, 2, 1)])
    assert got["counts"].tolist() == counter({2: (3, 1, 3)}) and got["matched_gold"].tolist() == [[0, 0, 0]]


def test_a_span_starting_on_an_inner_piece_has_the_signature_of_the_whole_word():
    assert signature(WI[0], WK[0], 2, 3) == signature(WI[0], WK[0], 1, 3) == (7, 8)
    got = run([(2, 3, 1, 1), (5, 5, 1, 1)], [(1, 3, 1, 1), (4, 5, 1, 1)])
    assert got["counts"].tolist() == counter({1: (2, 2, 2)}) and got["matched_gold"].tolist() == [[0, 1]]
    # ... and equal to the same words further on: (6..8) is "ba ko" again
    assert run([(6, 8, 1, 1)], [(2, 3, 1, 1)])["matched_gold"].tolist() == [[0]]


def test_without_word_keys_the_word_index_is_the_key():
    pred, gold = [(6, 7, 2, 1), (2, 2, 2, 1)], [(1, 2, 2, 1)]
    assert run(pred, gold)["matched_gold"].tolist() == [[0, 0]]                       # by string: both are "ba"
    got = run(pred, gold, word_key=None)
    assert got["matched_gold"].tolist() == [[-1, 0]]                                  # by position: only word 0 itself
    assert got["counts"].tolist() == counter({2: (2, 1, 1)})


# ---- SpanScorer.compute ------------------------------------------------------------------------------------------------------
def test_compute_arithmetic_on_a_hand_set_counter():
    from mtvaf_amd.metrics import SpanScorer
    sc = SpanScorer()
    assert sc.classes == ("other", "neutral", "positive", "negative") and sc.counts.tolist() == [0] * 14
    #                          other     neutral   positive  negative  relevant_other sentences
    sc.counts = torch.tensor([3, 0, 0,   4, 2, 1,  0, 0, 0,  5, 10, 5,  2,            7])
    got = sc.compute()
    assert got["other"] == dict(retrieved=3, relevant=0, common=0, precision=0.0, recall=0.0, f1=0.0)
    assert got["neutral"] == dict(retrieved=4, relevant=2, common=1, precision=0.25, recall=0.5, f1=2 * 0.25 * 0.5 / 0.75)
    assert got["positive"] == dict(retrieved=0, relevant=0, common=0, precision=0.0, recall=0.0, f1=0.0)
    assert got["negative"] == dict(retrieved=5, relevant=10, common=5, precision=1.0, recall=0.5, f1=2 * 0.5 / 1.5)
    p, r = 6 / 12, 6 / 14
    assert got["micro"] == dict(p=p, r=r, f1=2 * p * r / (p + r), common=6, retrieved=12, relevant=14)
    # macro: over other, neutral, negative -- positive has no count
    assert got["macro"] == dict(precision=(0.0 + 0.25 + 1.0) / 3, recall=(0.0 + 0.5 + 0.5) / 3,
                                f1=(0.0 + got["neutral"]["f1"] + got["negative"]["f1"]) / 3)
    assert got["sentences"] == 7
    sc.reset()
    got = sc.compute()
    assert got["micro"] == dict(p=0.0, r=0.0, f1=0.0, common=0, retrieved=0, relevant=0)
    assert got["macro"] == dict(precision=0.0, recall=0.0, f1=0.0) and got["sentences"] == 0
    assert got["positive"]["f1"] == 0.0
    with pytest.raises(ValueError):
        SpanScorer(classes=("only",))


def test_compute_equals_eval_absa_on_the_fixture_counts():
    """eval_absa's p / r / f1 from its own counts: p = common / retrieved, r = common / relevant, f1 = 2pr / (p + r)."""
    from mtvaf_amd.metrics import SpanScorer
    for c, inp, (common, retrieved, relevant) in golden_cases():
        sc = SpanScorer()
        sc.counts = torch.from_numpy(C.score(**inp)["counts"])
        got = sc.compute()["micro"]
        p, r = common / retrieved, common / relevant
        assert got == dict(p=p, r=r, f1=2 * p * r / (p + r), common=common, retrieved=retrieved, relevant=relevant), c


# ---- the wrapper and the model switch ----------------------------------------------------------------------------------------
def test_symbol_exported_and_bound():
    from mtvaf_amd import hip
    assert "mtvaf_span_counts" in hip.exported_symbols()
    assert hip.lib().mtvaf_span_counts.argtypes == hip._SIGS["mtvaf_span_counts"][1] == abi_header.signature("mtvaf_span_counts")[1]
    assert "span_score.hip" in __import__("mtvaf_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("S,N,G,Kc", [(513, 4, 4, 4), (16, 33, 4, 4), (16, 4, 33, 4), (16, 4, 4, 1), (16, 4, 4, 9), (0, 4, 4, 4)])
def test_limits_are_checked_before_any_launch(S, N, G, Kc):
    """The library answers its shape status without touching the device; the Python layer raises ValueError."""
    from mtvaf_amd import hip
    rc = hip.lib().mtvaf_span_counts(*[None] * 10, 2, S, N, G, Kc, None, None, None, None)
    assert rc == -1
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int64)  # noqa: E731
    with pytest.raises(ValueError, match=f"S={S}" if S in (0, 513) else f"N={N}" if N == 33 else f"G={G}" if G == 33 else f"K={Kc}"):
        hip.span_counts(z(2, N), z(2, N), z(2, N), torch.zeros(2, N, Kc), z(2, G), z(2, G), z(2, G), z(2, G),
                        torch.zeros(2, S, dtype=torch.int32), None, z(3 * Kc + 2))


def test_mismatched_shapes_raise():
    from mtvaf_amd import hip
    from mtvaf_amd.metrics import SpanScorer
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int64)  # noqa: E731
    wi = torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(ValueError):  # a counter for another K
        hip.span_counts(z(2, 4), z(2, 4), z(2, 4), torch.zeros(2, 4, 4), z(2, 3), z(2, 3), z(2, 3), z(2, 3), wi, None, z(17))
    with pytest.raises(ValueError):  # gold masks of another width
        hip.span_counts(z(2, 4), z(2, 4), z(2, 4), torch.zeros(2, 4, 4), z(2, 3), z(2, 3), z(2, 3), z(2, 2), wi, None, z(14))
    with pytest.raises(ValueError):  # five class names, four logits
        SpanScorer(classes=("a", "b", "c", "d", "e")).update(
            dict(span_starts=z(2, 4), span_ends=z(2, 4), label_masks=z(2, 4), logits=torch.zeros(2, 4, 4)), z(2, 3), z(2, 3),
            z(2, 3), z(2, 3), wi)


def test_the_model_has_no_scorer_unless_asked():
    from transformers import BertConfig
    from mtvaf_amd.metrics import SpanScorer
    from mtvaf_amd.models.bert_model import TVNetSAModel
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=False, bert_config=BertConfig(
        vocab_size=50, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, max_position_embeddings=32))
    assert TVNetSAModel(["a"], None, args).span_scorer is None
    args.score_spans = False
    assert TVNetSAModel(["a"], None, args).span_scorer is None
    args.score_spans = True
    sc = TVNetSAModel(["a"], None, args).span_scorer
    assert isinstance(sc, SpanScorer) and sc.classes == ("other", "neutral", "positive", "negative")
