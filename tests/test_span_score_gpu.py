"""Aspect scoring on the MI355X: `mtvaf_span_counts` / `SpanScorer` against the restatement of its rule over the case table and
against the counts recorded from the reference's eval_absa, accumulation, determinism, graph capture, and `TVNetSAModel.predict`
with gold terms end to end.  The counter and the per-slot outputs are integers: every comparison is exact."""
import numpy as np
import pytest
import torch

import params as P
import span_score_cases as C
from test_model_gpu import DEV, hf_config, load, make_args, LABELS
from test_span_score import NAMES, golden_cases

pytestmark = pytest.mark.gpu


def on_device(inp, keyed=True):
    t = {k: torch.from_numpy(inp[k]).to(DEV) for k in NAMES}
    pred = {k: t[k] for k in ("span_starts", "span_ends", "label_masks", "logits")}
    gold = [t[k] for k in ("gold_starts", "gold_ends", "gold_class", "gold_masks")]
    return pred, gold, t["word_index"], t["word_key"] if keyed else None


def scorer(K):
    from mtvaf_amd.metrics import SpanScorer
    return SpanScorer(classes=[f"c{k}" for k in range(K)], device=DEV)


def run(sc, inp, keyed=True, slots=True):
    """one update -> (the counter after it, pred_class, matched_gold) as numpy arrays"""
    pred, gold, wi, wk = on_device(inp, keyed)
    out = sc.update(pred, *gold, wi, wk, return_slots=slots)
    return (sc.counts.cpu().numpy(), *(x.cpu().numpy() for x in (out or ())))


def assert_same(got, ref, what=""):
    counts, pred_class, matched_gold = got
    assert counts.dtype == np.int64 and counts.tolist() == ref["counts"].tolist(), (what, counts.tolist(), ref["counts"].tolist())
    for name, g in (("pred_class", pred_class), ("matched_gold", matched_gold)):
        assert g.dtype == np.int32 and g.shape == ref[name].shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, ref[name]), (what, name, np.argwhere(g != ref[name])[:4].tolist())


@pytest.mark.parametrize("case", C.TABLE, ids=[c[0] for c in C.TABLE])
def test_kernel_equals_restatement(case):
    name, B, S, N, G, K, keyed = case
    inp = C.make_inputs(B, S, N, G, K, seed=2000 + 7 * S + B)
    ref = C.score(**{**inp, "word_key": inp["word_key"] if keyed else None})
    assert_same(run(scorer(K), inp, keyed), ref, name)
    common, retrieved, relevant = C.totals(ref["counts"], K)
    assert retrieved >= N and relevant >= G and ref["counts"][3 * K + 1] == B  # row 0: every slot of both sides exists
    assert inp["gold_ends"][0, 0] - inp["gold_starts"][0, 0] + 1 == max(S - 2, 1)
    if B >= 3:
        assert (ref["pred_class"][1] == -1).all() and (ref["matched_gold"][2] == -1).all()
    if B == 70:
        assert 0 < common < retrieved


def test_kernel_equals_the_reference_counts_of_the_fixture():
    for c, inp, want in golden_cases():
        K = inp["logits"].shape[2]
        counts, pred_class, _ = run(scorer(K), inp)
        assert list(C.totals(counts, K)) == want, c
        assert np.array_equal(pred_class, np.where(inp["label_masks"] != 0, inp["logits"].argmax(2), -1)), c


def test_updates_accumulate_runs_repeat_reset_zeroes_and_slots_are_optional():
    one = C.make_inputs(37, 65, 20, 4, 4, seed=3)
    two = C.make_inputs(9, 130, 5, 32, 4, seed=4)
    sc = scorer(4)
    c1 = run(sc, one)[0].copy()
    sc.reset()
    assert not sc.counts.cpu().numpy().any()
    c2 = run(sc, two)[0].copy()
    assert c1.any() and c2.any()
    assert c1.tolist() == C.score(**one)["counts"].tolist() and c2.tolist() == C.score(**two)["counts"].tolist()
    sc.reset()
    again = run(sc, one)
    assert again[0].tolist() == c1.tolist(), "two runs of the same input differ"
    assert run(sc, two, slots=False)[0].tolist() == (c1 + c2).tolist()  # null per-slot pointers, onto the first batch's counts
    got = sc.compute()
    assert got["sentences"] == 37 + 9 and got["micro"]["retrieved"] == int((c1 + c2)[0:12:3].sum())
    assert got["c2"]["common"] == int((c1 + c2)[8])
    sc.reset()
    assert not sc.counts.cpu().numpy().any()
    # either per-slot output alone
    from mtvaf_amd import hip
    pred, gold, wi, wk = on_device(one)
    for which in (0, 1):
        slots = [None, None]
        slots[which] = torch.full((37, 20), -7, dtype=torch.int32, device=DEV)
        sc.reset()
        hip.span_counts(pred["span_starts"], pred["span_ends"], pred["label_masks"], pred["logits"], *gold, wi, wk, sc.counts, *slots)
        assert sc.counts.cpu().numpy().tolist() == c1.tolist()
        assert np.array_equal(slots[which].cpu().numpy(), again[1 + which])


def test_other_dtypes_are_cast_and_limits_raise_on_the_device_too():
    inp = C.make_inputs(5, 24, 5, 4, 4, seed=9)
    ref = C.score(**inp)
    pred, gold, wi, wk = on_device(inp)
    sc = scorer(4)
    out = sc.update({k: (v.int() if v.dtype == torch.int64 else v.double()) for k, v in pred.items()}, *[g.int() for g in gold],
                    wi.long(), wk.long(), return_slots=True)
    assert_same((sc.counts.cpu().numpy(), *(x.cpu().numpy() for x in out)), ref, "cast")
    sc.reset()
    z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="S=513"):
        sc.update(pred, *gold, z(5, 513, dtype=torch.int32))
    with pytest.raises(ValueError, match="G=33"):
        sc.update(pred, z(5, 33), z(5, 33), z(5, 33), z(5, 33), wi)
    assert not sc.counts.cpu().numpy().any()


def test_graph_capture_adds_on_every_replay():
    """One capture of `update` in a single-stream graph, replayed twice: no host sync in the call, the counter takes two batches."""
    inp = C.make_inputs(3, 64, 20, 4, 4, seed=5)
    ref = C.score(**inp)
    pred, gold, wi, wk = on_device(inp)
    sc = scorer(4)
    sc.update(pred, *gold, wi, wk, return_slots=True)  # library loaded, allocator warm
    torch.cuda.synchronize()
    sc.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slots = sc.update(pred, *gold, wi, wk, return_slots=True)
    sc.reset()  # whatever the capture itself did to the counter
    graph.replay()
    assert_same((sc.counts.cpu().numpy(), *(x.cpu().numpy() for x in slots)), ref, "replay 1")
    graph.replay()
    assert sc.counts.cpu().numpy().tolist() == (2 * ref["counts"]).tolist()
    assert ref["counts"][:12].any()


def test_predict_scores_its_own_spans():
    """TVNetSAModel.predict on the tiny config of the tvnet1_tiny_B3S16 fixture, eval mode.  With ``args.score_spans`` and gold
    terms the counter and the per-slot outputs are the restatement applied to the tensors the call returned (word map from the
    attention mask, as the proposal's); without gold the call returns the keys and bits of a model built without the switch."""
    from mtvaf_amd.models.bert_model import TVNetSAModel
    fx = load("tvnet1_tiny_B3S16")
    cfg = P.TINY_BERT_L8
    seed, B, S = int(fx["seed"]), int(fx["B"]), int(fx["S"])
    lengths = [int(x) for x in fx["lengths"]]
    sd = {**{"bert." + k: v for k, v in P.encoder_params(cfg, seed).items()}, **P.span_head_params(cfg, seed + 3)}

    def build(**kw):
        args = make_args(use_prefix=False, gcn_layer_number=0, num_layers=0, logit_threshold=-100.0, **kw)
        args.bert_config = hf_config(cfg)
        m = TVNetSAModel(LABELS, None, args)
        assert not m.load_state_dict(sd, strict=False)[1]
        return m.to(DEV).eval()

    plain, scored = build(), build(score_spans=True)
    assert plain.span_scorer is None and scored.span_scorer is not None
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, seed + 1, B, S, lengths))
    base = plain.predict(ids, mask, tt)
    same = scored.predict(ids, mask, tt)
    assert list(same) == list(base) and all(torch.equal(same[k], base[k]) for k in base)
    assert not scored.span_scorer.counts.any()  # nothing was counted (the counter has not even left the host)

    # gold terms from the first pass: slot 0 = predicted slot 0 with its class, slot 1 = predicted slot 1 with the next class,
    # slot 2 = a truncated term, slot 3 absent
    st, en = base["span_starts"].cpu().numpy(), base["span_ends"].cpu().numpy()
    cls = base["logits"].float().cpu().numpy().argmax(2)
    assert bool((base["label_masks"][:, :2] == 1).all())
    gold = dict(starts=np.stack([st[:, 0], st[:, 1], 0 * st[:, 0], st[:, 0]], 1), ends=np.stack([en[:, 0], en[:, 1], 0 * en[:, 0], en[:, 0]], 1),
                classes=np.stack([cls[:, 0], (cls[:, 1] + 1) % 4, cls[:, 0], cls[:, 0]], 1).astype(np.int64),
                masks=np.tile(np.array([1, 1, 1, 0], np.int64), (B, 1)))
    plain_gold = plain.predict(ids, mask, tt, gold={k: torch.from_numpy(v).to(DEV) for k, v in gold.items()})
    assert list(plain_gold) == list(base)  # no scorer: gold is ignored
    out = scored.predict(ids, mask, tt, gold={k: torch.from_numpy(v).to(DEV) for k, v in gold.items()})
    assert list(out) == list(base) + ["pred_class", "matched_gold"] and all(torch.equal(out[k], base[k]) for k in base)
    pos = np.where(mask.cpu().numpy() != 0, np.arange(S, dtype=np.int32)[None], -1).astype(np.int32)
    ref = C.score(out["span_starts"].cpu().numpy(), out["span_ends"].cpu().numpy(), out["label_masks"].cpu().numpy(),
                  out["logits"].cpu().numpy(), gold["starts"], gold["ends"], gold["classes"], gold["masks"], pos, None)
    assert_same((scored.span_scorer.counts.cpu().numpy(), out["pred_class"].cpu().numpy(), out["matched_gold"].cpu().numpy()), ref,
                "predict")
    got = scored.span_scorer.compute()
    assert got["sentences"] == B and got["micro"]["relevant"] == 3 * B and got["micro"]["common"] >= B  # slot 0 hits in every row
    assert (ref["matched_gold"][:, 0] == 0).all()
