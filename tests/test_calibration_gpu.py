"""Calibration counting on the MI355X: `mtvaf_chunk_calibration` / `mtvaf_entity_calibration` / `CalibrationScorer` against the
restatement of tests/calibration_cases.py (pinned by hand in test_calibration.py) at B = 3, S = 12, C = 7, W = 4, T = 3, NB = 8,
E = 6; adding, reset, determinism; the gold counts against `EntityScorer`; the model's opt-in; the argument checks.

Integer counters must be equal.  sum_p / sum_sq: rtol 1e-9 -- every term is non-negative and there are at most B S W T ~ 4e2 of
them; the device's and NumPy's float64 exp differ by a few ulp (~1e-16 each) and the order of summation adds at most n 2^-53
~ 5e-14: 1e-9 leaves six orders of margin and still catches an accumulation in float32 (~1e-7)."""
import numpy as np
import pytest
import torch

import calibration_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-9


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tables_dev(tables):
    return [dev(t.reshape(-1)) for t in tables]


def fields(block, T, NB):
    """The documented layout of the counter block -> (ints int64 [2 T NB + 2 T + 1], sum_p [T,NB], sum_sq [T,NB]) on the host"""
    b = block.cpu()
    c = T * NB
    ints = torch.cat([b[:2 * c + 2 * T], b[-1:]]).numpy()
    f = b[2 * c + 2 * T:4 * c + 2 * T].view(torch.float64).numpy()
    return ints, f[:c].reshape(T, NB), f[c:].reshape(T, NB)


def same(block, want, T=K.T, NB=K.NB):
    ints, sum_p, sum_sq = fields(block, T, NB)
    assert np.array_equal(ints, want.ints()), (ints.tolist(), want.ints().tolist())
    for name, got, ref in (("sum_p", sum_p, want.sum_p), ("sum_sq", sum_sq, want.sum_sq)):
        err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print(f"{name}: max rel err {float(np.where(ref != 0, err, 0).max()):.3e} (bound {RTOL:.0e})")
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


def events(lp, gold, mask, keep, edges, tables, block=None):
    from mtvaf_amd import hip
    block = torch.zeros(hip.calibration_words(lp.shape[3], len(edges) - 1), dtype=torch.int64, device=DEV) if block is None else block
    return hip.chunk_calibration(dev(lp), dev(gold), dev(mask), dev(keep), *tables_dev(tables), dev(edges), block)


def entities(ents, conf, gold, mask, keep, edges, tables, T=K.T, block=None):
    from mtvaf_amd import hip
    block = torch.zeros(hip.calibration_words(T, len(edges) - 1), dtype=torch.int64, device=DEV) if block is None else block
    return hip.entity_calibration(dev(ents), dev(conf), dev(gold), dev(mask), dev(keep), *tables_dev(tables), dev(edges), T, block)


# ---- the kernels against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_keep", [True, False])
def test_events_against_the_restatement(with_keep):
    lp, gold, mask, keep, edges = K.events_case()
    keep = keep if with_keep else None
    tables = K.strict_bio_tables()
    want = K.reference_events(lp, gold, mask, keep, tables, edges)
    # what the case was built to hold
    assert np.isnan(lp).any() and np.isinf(lp).any() and (lp == edges[4]).any() and mask[0].all() and mask[1].sum() == 1
    if with_keep:
        assert want.gold.tolist() == [0, 3, 1] and want.reach.tolist() == [0, 2, 1]  # the A of 5 kept columns is out of reach
        assert want.hit[1, 4] >= 1  # the hit that sits exactly on edge 4
    assert want.n.sum() == np.isfinite(lp).sum() and want.sentences == 3
    same(events(lp, gold, mask, keep, edges, tables), want)


@pytest.mark.parametrize("with_keep", [True, False])
def test_entities_against_the_restatement(with_keep):
    ents, conf, gold, mask, keep, edges = K.entities_case()
    keep = keep if with_keep else None
    tables = K.strict_bio_tables()
    want = K.reference_entities(ents, conf, gold, mask, keep, tables, edges, K.T)
    if with_keep:
        assert want.n.sum() == 9 and want.hit.sum() == 5 and want.n[:, 0].sum() == 2  # 11 used slots, 2 skipped; 2 without confidence
        assert want.gold.tolist() == want.reach.tolist() == [0, 3, 1]
        assert want.hit[2].sum() == 2  # the duplicate hits twice
    same(entities(ents, conf, gold, mask, keep, edges, tables), want)


def test_more_types_than_one_pass_holds():
    """T = 9 at NB = 64: three passes of four types (256 cells each) and a part-filled last one."""
    rng = np.random.default_rng(5)
    T, NB, S, W = 9, 64, 70, 3
    start, end, type_of = K.strict_bio_tables()
    type_of = np.array([0, 0, 3, 3, 8, 8, 0, 0], np.int32)
    edges = K.edges_for(NB)
    gold = rng.choice([K.O, K.BA, K.IA, K.BB, K.IB], size=(2, S)).astype(np.int64)
    mask = np.ones((2, S), np.uint8)
    mask[1, 66:] = 0
    lp = np.log(rng.uniform(1e-4, 1.0, (2, S, W, T))).astype(np.float32)
    lp[rng.random(lp.shape) < 0.5] = -np.inf
    want = K.reference_events(lp, gold, mask, None, (start, end, type_of), edges)
    assert want.hit.sum() > 0 and want.gold[3] > 0 and want.gold[8] > 0
    same(events(lp, gold, mask, None, edges, (start, end, type_of)), want, T, NB)


# ---- adding, reset, determinism ------------------------------------------------------------------------------------------------
def test_two_calls_add_and_the_same_call_gives_the_same_bits():
    tables = K.strict_bio_tables()
    lp, gold, mask, keep, edges = K.events_case()
    lp2 = K.events_case(seed=1)[0]
    want = K.reference_events(lp, gold, mask, keep, tables, edges)
    want = K.reference_events(lp2, gold, mask, None, tables, edges, out=want)
    block = events(lp, gold, mask, keep, edges, tables)
    first = block.clone()
    events(lp2, gold, mask, None, edges, tables, block=block)
    same(block, want)
    again = events(lp, gold, mask, keep, edges, tables)
    assert torch.equal(first, again)  # the doubles too: they are compared as the words they are stored in
    ents, conf, gold, mask, keep, edges = K.entities_case()
    a, b = (entities(ents, conf, gold, mask, keep, edges, tables) for _ in range(2))
    assert torch.equal(a, b) and a.any()


LMAP = {n: i for i, n in enumerate(["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"], 1)}


def test_scorer_adds_resets_and_counts_the_gold_chunks_entity_scorer_counts():
    from mtvaf_amd.metrics import CalibrationScorer, EntityScorer, entity_tables
    rng = np.random.default_rng(11)
    gold, mask = K.valid_bio(rng, LMAP, 3, 12)
    sc, es = CalibrationScorer(LMAP, n_bins=8), EntityScorer(LMAP)
    T = len(sc.types)
    ents = np.full((3, 6, 3), -1, np.int32)
    ents[:, 0] = rng.integers(1, 11, (3, 3))
    conf = np.log(rng.uniform(0.01, 1, (3, 6))).astype(np.float32)
    for _ in range(2):
        sc.update_entities(dev(ents), dev(conf), dev(gold), dev(mask))
    es.update(dev(gold.astype(np.int32)), dev(gold), dev(mask))
    n, hit, g, reach, _, _, sentences = sc._fields(sc.block.cpu())
    assert int(sentences) == 6 and torch.equal(g, reach) and int(g.sum()) > 0
    assert (g // 2).tolist() == es.counts.cpu()[1:3 * T:3].tolist()  # per type, the gold chunks of the same labels, mask and tables
    # against the restatement over the scorer's own tables, gold X / [SEP] columns left out
    t = entity_tables(LMAP)
    keep = np.cumprod(mask, axis=1).astype(bool) & ~np.isin(gold, [LMAP["X"], LMAP["[SEP]"]])
    keep[:, 0] = False
    tables = (t["start"], t["end"], t["type_of"])
    want = K.reference_entities(ents, conf, gold, mask, keep.astype(np.uint8), tables, sc.edges.numpy(), T)
    want = K.reference_entities(ents, conf, gold, mask, keep.astype(np.uint8), tables, sc.edges.numpy(), T, out=want)
    same(sc.block, want, T, 8)
    with pytest.raises(ValueError):
        sc.update_events(torch.zeros(3, 12, 4, T, device=DEV), dev(keep.astype(np.uint8)), dev(gold), dev(mask))
    sc.reset()
    assert not sc.block.any()


# ---- the model -----------------------------------------------------------------------------------------------------------------
def model_batch(cfg, seed, B=3, S=12):
    import params as P
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, seed, B, S, lo_id=5))
    gold, _ = K.valid_bio(np.random.default_rng(seed), LMAP, B, S)
    lens = mask.sum(1).tolist()
    for r, L in enumerate(lens):  # the labels of a sentence of this batch's lengths: [CLS] ... [SEP], PAD behind
        gold[r, L - 1:] = 0
        gold[r, L - 1] = LMAP["[SEP]"]
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt), dev(gold)


def test_predict_posteriors_scores_its_events():
    from test_entity_counts_gpu import tiny_model
    from mtvaf_amd.metrics import entity_tables
    cfg, plain = tiny_model(max_entity_width=4)
    _, scored = tiny_model(max_entity_width=4, score_calibration="events", calibration_bins=8)
    assert plain.calibration_scorer is None and scored.calibration_scorer.n_bins == 8
    scored.load_state_dict(plain.state_dict())
    sc = scored.calibration_scorer
    t = entity_tables(LMAP)
    tables, T, want = (t["start"], t["end"], t["type_of"]), len(sc.types), None
    for step in range(2):
        kw, gold = model_batch(cfg, 70 + step)
        a, b = plain.predict_posteriors(**kw), scored.predict_posteriors(labels=gold, **kw)
        for k in ("log_post", "logz_a", "keep"):
            assert torch.equal(a[k], b[k]), k
        for k in ("entities", "log_confidence", "chunk_log_conf", "count"):
            assert torch.equal(a["decoded"][k], b["decoded"][k]) and (k == "chunk_log_conf" or torch.equal(a["selected"][k], b["selected"][k])), k
        want = K.reference_events(b["log_post"].cpu().numpy(), gold.cpu().numpy(), kw["attention_mask"].cpu().numpy(),
                                  b["keep"].cpu().numpy(), tables, sc.edges.numpy(), out=want)
    assert sc.kind == "events" and want.n.sum() > 0 and want.gold.sum() > 0
    same(sc.block, want, T, 8)
    r = sc.compute()
    assert r["sentences"] == 6 and r["micro"]["predicted"][0] == int(want.n.sum()) and r["pooled"]["gold"] == int(want.gold.sum())
    before = sc.block.clone()
    c = scored.predict_posteriors(**kw)  # without labels: nothing is counted, the tensors are the plain model's
    assert torch.equal(sc.block, before) and torch.equal(c["log_post"], a["log_post"])
    scored.predict(labels=gold, **kw)    # the scorer scores events: the entity lists pass it by
    assert torch.equal(sc.block, before)


@pytest.mark.parametrize("head", ["crf", "softmax"])
def test_predict_scores_its_entities(head):
    from test_entity_counts_gpu import tiny_model
    from mtvaf_amd.metrics import entity_tables
    cfg, plain = tiny_model(tag_head=head, max_entities=6)
    _, scored = tiny_model(tag_head=head, max_entities=6, score_calibration="entities", calibration_bins=8)
    scored.load_state_dict(plain.state_dict())
    sc = scored.calibration_scorer
    t = entity_tables(LMAP)
    tables, T, want = (t["start"], t["end"], t["type_of"]), len(sc.types), None
    for step in range(2):
        kw, gold = model_batch(cfg, 80 + step)
        a, b = plain.predict(**kw), scored.predict(labels=gold, **kw)
        for k in ("tags", "entities", "log_confidence", "confidence", "count"):
            assert torch.equal(a[k], b[k]), k
        g, m = gold.cpu().numpy(), kw["attention_mask"].cpu().numpy()
        keep = np.cumprod(m, axis=1).astype(bool) & ~np.isin(g, [LMAP["X"], LMAP["[SEP]"]])
        keep[:, 0] = False
        want = K.reference_entities(b["entities"].cpu().numpy(), b["log_confidence"].cpu().numpy(), g, m, keep.astype(np.uint8),
                                    tables, sc.edges.numpy(), T, out=want)
    assert sc.kind == "entities" and want.gold.sum() > 0
    same(sc.block, want, T, 8)
    assert sc.compute()["sentences"] == 6
    before = sc.block.clone()
    scored.predict(**kw)
    assert torch.equal(sc.block, before)
    if head == "softmax":
        with pytest.raises(ValueError, match="softmax"):
            tiny_model(tag_head=head, score_calibration="events")


# ---- arguments: refused before any launch --------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    from mtvaf_amd import hip
    lib = hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()

    def chunk(S=12, NB=8, W=4, wsb=None):
        need = lib.mtvaf_calibration_workspace_bytes(3, 3, NB)
        return lib.mtvaf_chunk_calibration(p, p, p, None, p, p, p, p, 3, S, 7, 3, W, NB, p, p, need if wsb is None else wsb, None)

    def entity(S=12, NB=8, E=6, wsb=None):
        need = lib.mtvaf_calibration_workspace_bytes(3, 3, NB)
        return lib.mtvaf_entity_calibration(p, p, p, p, None, p, p, p, p, 3, S, 7, 3, E, NB, p, p, need if wsb is None else wsb, None)
    assert chunk(S=513) == entity(S=513) == -1
    assert chunk(NB=65) == entity(NB=65) == chunk(W=17) == entity(E=65) == -3
    short = lib.mtvaf_calibration_workspace_bytes(3, 3, 8) - 1
    assert chunk(wsb=short) == entity(wsb=short) == -4
    assert lib.mtvaf_chunk_calibration(p, p, p, None, p, p, p, p, 3, 12, 7, 3, 4, 8, p, None, 1 << 20, None) == -4
    torch.cuda.synchronize()
    assert not buf.any()  # nothing ran
    with pytest.raises(ValueError):
        hip.chunk_calibration(torch.zeros(3, 12, 17, 3, device=DEV), buf[:36].view(3, 12), buf[:36].view(3, 12).to(torch.uint8), None,
                              *tables_dev(K.strict_bio_tables()), dev(K.edges_for(8)), buf[:hip.calibration_words(3, 8)])
