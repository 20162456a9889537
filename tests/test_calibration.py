"""Calibration scoring without a GPU: the restatement of the counting contract (tests/calibration_cases.py) on a sentence worked by
hand, and `CalibrationScorer.compute` on counter blocks written by hand or by the restatement -- curves, the tie rule of the best
threshold, ECE / Brier, the recall ceiling; the default edges; one kind of update per instance; the declarations."""
import numpy as np
import pytest
import torch

import abi_header
import calibration_cases as K

LMAP = {"O": 1, "B-A": 2, "I-A": 3, "B-B": 4, "I-B": 5, "X": 6, "[SEP]": 7}


def scorer(**kw):
    from mtvaf_amd.metrics import CalibrationScorer
    return CalibrationScorer(LMAP, **kw)


def load(sc, counts):
    """A restated Counts (or any object with its arrays) -> the scorer's block, through the documented layout"""
    n, hit, gold, reach, sum_p, sum_sq, sentences = sc._fields()
    for view, arr in ((n, counts.n), (hit, counts.hit), (gold, counts.gold), (reach, counts.reach), (sum_p, counts.sum_p),
                      (sum_sq, counts.sum_sq)):
        view.copy_(torch.from_numpy(np.asarray(arr)))
    sentences.fill_(counts.sentences)
    return sc


def test_restatement_on_a_hand_worked_sentence():
    """PAD B-A I-A O B-B X, columns 1..5 kept: the gold chunks are A over 1..2 and B at 4.  Five finite events, W = 2, 4 bins."""
    tables, edges = K.strict_bio_tables(), K.edges_for(4)
    gold = np.array([[K.PAD, K.BA, K.IA, K.O, K.BB, K.X]], np.int64)
    mask = np.ones((1, 6), np.uint8)
    lp = np.full((1, 6, 2, 3), -np.inf, np.float32)
    lp[0, 1, 1, 1] = np.log(0.9)   # A over 1..2: a hit, bin 3
    lp[0, 1, 0, 1] = np.log(0.3)   # A at 1 alone: a miss, bin 1
    lp[0, 4, 0, 2] = np.log(0.6)   # B at 4: a hit, bin 2
    lp[0, 4, 0, 1] = np.log(0.1)   # A at 4: the wrong type, bin 0
    lp[0, 2, 0, 0] = edges[2]      # exactly log 0.5: bin 2, a miss
    got = K.reference_events(lp, gold, mask, None, tables, edges)
    assert got.n.tolist() == [[0, 0, 1, 0], [1, 1, 0, 1], [0, 0, 1, 0]]
    assert got.hit.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]]
    assert got.gold.tolist() == got.reach.tolist() == [0, 1, 1] and got.sentences == 1
    f = lambda p: float(np.exp(np.float64(np.float32(np.log(p)))))  # noqa: E731  (the fp32 log is what is stored)
    np.testing.assert_allclose(got.sum_p, [[0, 0, 0.5, 0], [f(0.1), f(0.3), 0, f(0.9)], [0, 0, f(0.6), 0]], rtol=1e-7)
    np.testing.assert_allclose(got.sum_sq, [[0, 0, 0.25, 0], [f(0.1) ** 2, f(0.3) ** 2, 0, (f(0.9) - 1) ** 2], [0, 0, (f(0.6) - 1) ** 2, 0]],
                               rtol=1e-6)
    # the same chunks as listed entities: no width limit, a duplicate counts twice, an unopened I-B is no gold chunk
    gold2 = np.array([[K.PAD, K.IB, K.O, K.BA, K.IA, K.X]], np.int64)
    ents = np.array([[[3, 4, 1], [3, 4, 1], [1, 1, 2], [-1, -1, -1]]], np.int32)
    conf = np.log(np.array([[0.9, 0.2, 0.8, 1.0]], np.float32))
    got = K.reference_entities(ents, conf, gold2, mask, None, tables, edges, 3)
    assert got.n.tolist() == [[0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 1]] and got.hit.tolist() == [[0] * 4, [1, 0, 0, 1], [0] * 4]
    assert got.gold.tolist() == got.reach.tolist() == [0, 1, 0]


def hand_table(sc):
    """Two types over 4 bins, small enough to do on paper (see test_compute_on_a_hand_table)"""
    n, hit, gold, reach, sum_p, sum_sq, sentences = sc._fields()
    a, b = sc.types.index("A"), sc.types.index("B")
    n[a], hit[a] = torch.tensor([10, 2, 0, 4]), torch.tensor([0, 1, 0, 3])
    n[b], hit[b] = torch.tensor([0, 0, 2, 0]), torch.tensor([0, 0, 1, 0])
    gold[a], gold[b], reach[a], reach[b] = 5, 2, 4, 2
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    sum_p[a], sum_p[b] = f64([0.5, 0.7, 0.0, 3.2]), f64([0.0, 0.0, 1.2, 0.0])
    sum_sq[a], sum_sq[b] = f64([0.1, 0.4, 0.0, 0.5]), f64([0.0, 0.0, 0.5, 0.0])
    sentences.fill_(9)
    return sc


def test_compute_on_a_hand_table():
    from mtvaf_amd.metrics import calibration_to_rows
    sc = hand_table(scorer(n_bins=4))
    r = sc.compute()
    # pooled: n = 10 2 2 4, hits = 0 1 1 3, gold = 7
    assert r["pooled"]["bins"]["count"] == [10, 2, 2, 4] and r["pooled"]["bins"]["hits"] == [0, 1, 1, 3]
    assert r["micro"]["predicted"] == [18, 8, 6, 4] and r["micro"]["correct"] == [5, 5, 4, 3]
    assert r["micro"]["precision"] == pytest.approx([5 / 18, 5 / 8, 4 / 6, 3 / 4], rel=1e-12)
    assert r["micro"]["recall"] == pytest.approx([5 / 7, 5 / 7, 4 / 7, 3 / 7], rel=1e-12)
    assert r["micro"]["f1"] == pytest.approx([10 / 25, 10 / 15, 8 / 13, 6 / 11], rel=1e-12)
    assert r["best_k"] == 1 and r["best_f1"] == pytest.approx(2 / 3) and r["best_threshold"] == pytest.approx(0.25, rel=1e-6)
    # bins >= 1, N = 8: |0.5 - 0.35| 2/8 + |0.5 - 0.6| 2/8 + |0.75 - 0.8| 4/8; (0.4 + 0.5 + 0.5) / 8
    assert r["ece"] == pytest.approx(0.0875, rel=1e-12) and r["brier"] == pytest.approx(0.175, rel=1e-12)
    assert r["pooled"]["bins"]["accuracy"] == pytest.approx([0, 0.5, 0.5, 0.75]) and \
        r["pooled"]["bins"]["confidence"] == pytest.approx([0.05, 0.35, 0.6, 0.8])
    # every bin, N = 18: + |0 - 0.05| 10/18; (0.1 + 0.4 + 0.5 + 0.5) / 18
    r0 = sc.compute(first_bin=0)
    assert r0["ece"] == pytest.approx((0.05 * 10 + 0.15 * 2 + 0.1 * 2 + 0.05 * 4) / 18, rel=1e-12)
    assert r0["brier"] == pytest.approx(1.5 / 18, rel=1e-12)
    assert r["recall_ceiling"] == pytest.approx(6 / 7) and r["types"]["A"]["recall_ceiling"] == 0.8 and r["sentences"] == 9
    assert r["types"]["A"]["curve"]["predicted"] == [16, 6, 4, 4] and r["types"]["B"]["curve"]["correct"] == [1, 1, 1, 0]
    assert r["thresholds"][0] == 0.0 and r["thresholds"][-1] == 1.0
    rows = calibration_to_rows(r)
    assert all(type(v) in (int, float, str) for row in rows for v in row.values())
    pooled = [row for row in rows if row["table"] == "bins" and row["type"] == "pooled"]
    assert [row["count"] for row in pooled] == [10, 2, 2, 4] and pooled[1]["low"] == pytest.approx(0.25, rel=1e-6)
    micro = [row for row in rows if row["table"] == "curve" and row["type"] == "micro"]
    assert [row["predicted"] for row in micro] == [18, 8, 6, 4] and micro[0]["threshold"] == 0.0


def test_best_threshold_takes_the_lowest_edge_among_ties():
    sc = scorer(n_bins=4)
    n, hit, gold, *_ = sc._fields()
    a = sc.types.index("A")
    n[a], hit[a], gold[a] = torch.tensor([5, 0, 3, 0]), torch.tensor([0, 0, 3, 0]), 3
    r = sc.compute()
    assert r["micro"]["f1"] == pytest.approx([6 / 11, 1.0, 1.0, 0.0])  # bin 1 is empty: edges 1 and 2 predict the same items
    assert r["best_k"] == 1 and r["best_f1"] == 1.0 and r["best_threshold"] == pytest.approx(0.25, rel=1e-6)
    sc.reset()
    assert not sc.block.any() and sc.compute()["best_k"] == 0  # nothing scored: every F1 is 0, the lowest edge


def test_curves_fall_and_the_ceiling_is_below_one_when_gold_is_wider_than_the_widths():
    from mtvaf_amd.metrics import entity_tables
    sc = scorer(n_bins=8)
    t = entity_tables(LMAP)
    tables = (t["start"], t["end"], t["type_of"])
    rng = np.random.default_rng(3)
    gold = np.full((2, 12), LMAP["O"], np.int64)
    gold[0, 1], gold[0, 2:6], gold[0, 8] = LMAP["B-A"], LMAP["I-A"], LMAP["B-B"]  # A is 5 columns wide; W = 4
    gold[1, 3], gold[1, 4] = LMAP["B-B"], LMAP["I-B"]
    mask = np.ones((2, 12), np.uint8)
    T = len(sc.types)
    lp = np.log(rng.uniform(1e-3, 1, (2, 12, 4, T))).astype(np.float32)
    lp[rng.random(lp.shape) < 0.5] = -np.inf
    lp[0, 8, 0, sc.types.index("B")] = np.log(0.9)
    got = K.reference_events(lp, gold, mask, None, tables, sc.edges.numpy())
    a, b = sc.types.index("A"), sc.types.index("B")
    assert got.gold[a] == 1 and got.reach[a] == 0 and got.gold[b] == got.reach[b] == 2
    r = load(sc, got).compute()
    assert r["recall_ceiling"] == pytest.approx(2 / 3) and r["types"]["A"]["recall_ceiling"] == 0.0
    for sec in [r["pooled"]] + list(r["types"].values()):
        for key in ("predicted", "correct"):
            v = sec["curve"][key]
            assert all(x >= y for x, y in zip(v, v[1:])), (key, v)
        assert max(sec["curve"]["recall"], default=0) <= sec["recall_ceiling"] + 1e-12
    assert r["micro"]["predicted"][0] == int(np.isfinite(lp).sum()) and r["sentences"] == 2


def test_default_edges_and_given_edges():
    from mtvaf_amd.metrics import CalibrationScorer
    sc = scorer()
    e = sc.edges.numpy()
    assert sc.n_bins == 20 and e.dtype == np.float32 and e.shape == (21,) and e[0] == -np.inf and e[20] == 0.0
    assert np.array_equal(e[1:20], np.log(np.arange(1, 20) / 20).astype(np.float32))
    assert np.array_equal(scorer(n_bins=8).edges.numpy(), K.edges_for(8))
    sc = CalibrationScorer(LMAP, edges=[-np.inf, -2.0, -1.0, 0.0])
    assert sc.n_bins == 3 and sc.block.numel() == 4 * len(sc.types) * 3 + 2 * len(sc.types) + 1
    for bad in ([-np.inf, -1.0, -2.0, 0.0], [0.0], list(range(-66, 0))):
        with pytest.raises(ValueError):
            CalibrationScorer(LMAP, edges=bad)
    with pytest.raises(ValueError):
        scorer().compute(first_bin=21)


def test_one_kind_of_update_per_instance():
    lab, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.uint8)
    sc = scorer(n_bins=4)
    sc.kind = "events"  # as after an update_events
    with pytest.raises(ValueError, match="events"):
        sc.update_entities(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2), lab, mask)
    sc = scorer(n_bins=4)
    sc.kind = "entities"
    with pytest.raises(ValueError, match="entities"):
        sc.update_events(torch.zeros(1, 4, 2, len(sc.types)), mask, lab, mask)
    with pytest.raises(ValueError):  # the type axis must be the scheme's
        scorer(n_bins=4).update_events(torch.zeros(1, 4, 2, 3), mask, lab, mask)


def test_model_switch_is_checked_at_construction():
    import types
    from mtvaf_amd.models import bert_model as M
    labels = ["O", "B-A", "I-A", "X", "[CLS]", "[SEP]"]
    assert M._calibration_scorer(types.SimpleNamespace(), labels, "crf") is None
    sc = M._calibration_scorer(types.SimpleNamespace(score_calibration="events", calibration_bins=8), labels, "crf")
    assert sc.n_bins == 8 and sc.kind is None
    assert M._calibration_scorer(types.SimpleNamespace(score_calibration="entities"), labels, "softmax").n_bins == 20
    with pytest.raises(ValueError, match="softmax"):
        M._calibration_scorer(types.SimpleNamespace(score_calibration="events"), labels, "softmax")
    with pytest.raises(ValueError):
        M._calibration_scorer(types.SimpleNamespace(score_calibration="spans"), labels, "crf")


def test_declarations():
    import ctypes
    from mtvaf_amd import hip
    from mtvaf_amd.build import SOURCES
    names = ("mtvaf_calibration_workspace_bytes", "mtvaf_chunk_calibration", "mtvaf_entity_calibration")
    assert "calibration.hip" in SOURCES and set(names) <= set(hip.exported_symbols())
    for name in names:
        res, args = hip._SIGS[name]
        assert (res, list(args)) == abi_header.signature(name)
    assert [n for _, n in abi_header.prototype("mtvaf_chunk_calibration")[2]] == [
        "log_post", "gold", "mask", "keep", "start_tab", "end_tab", "type_of", "edges", "B", "S", "C", "n_types", "max_width",
        "n_bins", "counter", "workspace", "workspace_bytes", "stream"]
    comment = " ".join(abi_header.comment_before("mtvaf_calibration_workspace_bytes").replace("\n *", "\n").split())
    for phrase in ("lp >= edges[k]", "gold_reachable", "sum_sq", "MTVAF_ERR_WORKSPACE", "-inf and NaN elements are skipped",
                   "bin 0 with p = 0", "an end without a start is dropped", "stream capture"):
        assert phrase in comment, phrase
    lib = hip.lib()
    assert lib.mtvaf_calibration_workspace_bytes(3, 3, 8) == 3 * (4 * 3 * 8 + 2 * 3) * 8
    assert lib.mtvaf_calibration_workspace_bytes(3, 65, 8) == lib.mtvaf_calibration_workspace_bytes(3, 3, 65) == 0
    assert hip.calibration_words(3, 8) == 4 * 3 * 8 + 2 * 3 + 1
    assert ctypes.sizeof(ctypes.c_double) == ctypes.sizeof(ctypes.c_int64) == 8
