"""n-best Viterbi on the MI355X: `mtvaf_crf_nbest` / `CRF.decode_nbest` / `TVNetSAModel2.predict_nbest` against the float64
references of tests/crf_nbest_cases.py.  Scores are held to delta = 2^-24 (2 len + 1) max|score| whatever the tags (it holds under
near-ties), tags to the reference exactly on the gapped cases; every figure is printed as err / bound before it is asserted."""
import numpy as np
import pytest
import torch

import crf_nbest_cases as N
import params as P
import test_crf_entities_gpu as T  # (its tiny model configuration)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ident(c):
    return "C{}-S{}-K{}-B{}-seed{}".format(*c)


def run(inp, K=None, return_logprob=True):
    crf = T.make_crf(inp.start, inp.end, inp.trans)
    res = crf.decode_nbest(inp.em.to(DEV), inp.mask.to(DEV), nbest=inp.K if K is None else K, return_logprob=return_logprob)
    return crf, res, {k: v.cpu().numpy() for k, v in res.items() if v is not None}


def check_properties(what, ref, r):
    """Everything that holds for every case, near-ties included."""
    inp, K = ref.inp, r["tags"].shape[1]
    B, S, C = inp.em.shape
    assert r["tags"].shape == (B, K, S) and r["scores"].shape == r["logprob"].shape == (B, K) and r["n_paths"].shape == (B,)
    worst = dict(score=0.0, rescore=0.0, logprob=0.0)
    for b, s in enumerate(ref.sents):
        n, tags, sc, lp = s.n_paths, r["tags"][b], r["scores"][b].astype(np.float64), r["logprob"][b].astype(np.float64)
        assert r["n_paths"][b] == n == min(K, C ** s.n), what
        assert (tags[n:] == -1).all() and (sc[n:] == -np.inf).all() and (lp[n:] == -np.inf).all(), what
        assert (tags[:n, s.n:] == -1).all() and (tags[:n, :s.n] >= 0).all() and (tags[:n, :s.n] < C).all(), what
        assert np.isfinite(sc[:n]).all() and (np.diff(sc[:n]) <= 0).all(), what
        assert len({tuple(row) for row in tags[:n, :s.n].tolist()}) == n, what
        own = np.array([N.path_score(ref.em[b], ref.start, ref.end, ref.trans, row) for row in tags[:n, :s.n].tolist()])
        worst["score"] = max(worst["score"], np.abs(sc[:n] - s.scores).max() / s.delta)
        worst["rescore"] = max(worst["rescore"], np.abs(sc[:n] - own).max() / s.delta)
        worst["logprob"] = max(worst["logprob"], np.abs(lp[:n] - (s.scores - s.logz)).max() / (s.delta + ref.logz_bound))
        assert np.exp(lp[:n]).sum() <= 1 + 1e-5, what
    print(f"crf-nbest {what}: err / bound score {worst['score']:.3f} rescore {worst['rescore']:.3f} logprob {worst['logprob']:.3f}")
    assert worst["score"] <= 1.0 and worst["rescore"] <= 1.0 and worst["logprob"] <= 1.0, (what, worst)


@pytest.mark.parametrize("case", N.CASES, ids=ident)
def test_every_case(case):
    ref = N.reference(case)
    check_properties(ident(case), ref, run(ref.inp)[2])


@pytest.mark.parametrize("case", N.GAPPED, ids=ident)
def test_gapped_cases_return_the_reference_paths(case):
    ref = N.reference(case)
    crf, res, r = run(ref.inp)
    check_properties(ident(case), ref, r)
    for b, s in enumerate(ref.sents):
        assert r["tags"][b, :s.n_paths, :s.n].tolist() == s.paths, (case, b)
    # rank 0 is the one-best decoder's answer, and the K = 1 call's to the bit
    tags1, lens1 = crf.decode_packed(ref.inp.em.to(DEV), ref.inp.mask.to(DEV))
    assert torch.equal(res["tags"][:, 0], tags1) and lens1.cpu().tolist() == ref.inp.lengths
    _, one, _ = run(ref.inp, K=1)
    assert torch.equal(one["tags"][:, 0], res["tags"][:, 0]) and torch.equal(one["scores"][:, 0], res["scores"][:, 0])
    assert torch.equal(one["logprob"][:, 0], res["logprob"][:, 0]) and bool((one["n_paths"] == 1).all())


def test_equal_scores_come_in_the_order_of_the_tie_rule():
    inp = N.tie_inputs()
    _, _, r = run(inp)
    assert r["n_paths"].tolist() == [8] and r["tags"][0, :, :2].tolist() == N.TIE_ORDER[:8]  # (the ninth is past K = 8)
    assert (r["tags"][0, :, 2] == -1).all() and (r["scores"] == 0).all()
    assert np.allclose(r["logprob"], -np.log(9.0), rtol=0, atol=1e-6)
    _, _, r3 = run(inp, K=3)
    assert r3["tags"][0, :, :2].tolist() == N.TIE_ORDER[:3]


def test_without_logprob_and_into_given_tensors():
    from mtvaf_amd import hip
    case = (13, 16, 8, 5, 1)
    ref = N.reference(case)
    crf, res, r = run(ref.inp)
    _, bare, _ = run(ref.inp, return_logprob=False)
    assert bare["logprob"] is None
    for k in ("tags", "scores", "n_paths"):
        assert torch.equal(bare[k], res[k]), k
    out = (torch.full((5, 8, 16), 12345, dtype=torch.int32, device=DEV), torch.full((5, 8), float("nan"), device=DEV),
           torch.full((5, 8), float("nan"), device=DEV), torch.full((5,), -7, dtype=torch.int32, device=DEV))
    got = hip.crf_nbest(ref.inp.em.to(DEV), ref.inp.mask.to(DEV), crf.start_transitions.data, crf.end_transitions.data,
                        crf.transitions.data, 8, out=out)
    assert got[0] is out[0]
    for k, o in zip(("tags", "scores", "logprob", "n_paths"), out):
        assert torch.equal(res[k], o), k  # (bit for bit: every element is written)


def test_batch_first_false_takes_time_major_inputs():
    from mtvaf_amd.modules.crf import CRF
    ref = N.reference((5, 7, 4, 5, 0))
    crf, res, _ = run(ref.inp)
    tm = CRF(5, batch_first=False).to(DEV)
    tm.load_state_dict(crf.state_dict())
    got = tm.decode_nbest(ref.inp.em.to(DEV).transpose(0, 1), ref.inp.mask.to(DEV).transpose(0, 1), nbest=4)
    for k in ("tags", "scores", "logprob", "n_paths"):
        assert torch.equal(got[k], res[k]), k


def test_nbest_to_lists_reads_the_device_result():
    from mtvaf_amd.metrics import nbest_to_lists
    ref = N.reference((3, 2, 8, 5, 0))
    _, res, r = run(ref.inp)
    lists = nbest_to_lists(res)
    assert [len(x) for x in lists] == [s.n_paths for s in ref.sents]
    for b, s in enumerate(ref.sents):
        assert [h[0] for h in lists[b]] == s.paths
        assert [h[1] for h in lists[b]] == r["scores"][b, :s.n_paths].tolist()
        assert np.allclose([h[2] for h in lists[b]], np.exp(r["logprob"][b, :s.n_paths].astype(np.float64)), rtol=1e-12)


def test_graph_capture_replays_to_the_same_bits():
    """One capture of `CRF.decode_nbest` (forward recursion + n-best kernel) replayed on the captured emissions and on new ones
    written in place: no host sync, no allocation the graph's pool does not own."""
    ref, ref2 = N.reference((13, 16, 8, 5, 1)), N.reference((13, 16, 8, 5, 7))
    crf = T.make_crf(ref.inp.start, ref.inp.end, ref.inp.trans)
    buf, mask_d = ref.inp.em.to(DEV).clone(), ref.inp.mask.to(DEV)
    crf.decode_nbest(buf, mask_d, nbest=8)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crf.decode_nbest(buf, mask_d, nbest=8)
    seen = []
    for em in (ref.inp.em, ref2.inp.em):
        buf.copy_(em)
        eager = crf.decode_nbest(buf, mask_d, nbest=8)
        graph.replay()
        for k in ("tags", "scores", "logprob", "n_paths"):
            assert torch.equal(out[k], eager[k]), k
        seen.append(out["tags"].cpu().clone())
    assert not torch.equal(seen[0], seen[1])
    check_properties("replay", ref, {k: v.cpu().numpy() for k, v in
                                     crf.decode_nbest(ref.inp.em.to(DEV), mask_d, nbest=8).items()})


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_prefix", [False, True])
def test_predict_nbest(use_prefix):
    from mtvaf_amd import engine
    cfg, m = T.tiny_model(use_prefix, max_entities=16)
    B, S, K = 6, 32, 4
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt)
    if use_prefix:
        g = torch.Generator().manual_seed(52)
        kw.update(images=torch.rand(B, 3840, 2, 2, generator=g).to(DEV), aux_imgs=torch.rand(B, 3, 3840, 2, 2, generator=g).to(DEV))
    m.train()
    offset = engine.RNG.offset
    before = m.predict(**kw)
    res = m.predict_nbest(**kw, nbest=K)
    after = m.predict(**kw)
    assert m.training and engine.RNG.offset == offset
    for k in ("tags", "lengths", "entities", "log_confidence", "confidence", "count"):
        assert torch.equal(before[k], after[k]), k          # predict is what it was
        assert torch.equal(res[k][:, 0], before[k]), k      # hypothesis 0 is predict's answer, to the bit
    assert res["types"] == before["types"]
    E = 16
    assert tuple(res["tags"].shape) == (B, K, S) and tuple(res["scores"].shape) == tuple(res["logprob"].shape) == (B, K)
    assert tuple(res["entities"].shape) == (B, K, E, 3) and tuple(res["confidence"].shape) == tuple(res["log_confidence"].shape) == (B, K, E)
    assert tuple(res["count"].shape) == tuple(res["lengths"].shape) == (B, K) and tuple(res["n_paths"].shape) == (B,)
    assert bool((res["n_paths"] == K).all()) and int(before["count"].sum()) >= 3
    assert bool((res["scores"][:, :-1] >= res["scores"][:, 1:]).all()) and float(torch.exp(res["logprob"]).sum(1).max()) <= 1 + 1e-5
    assert m.predict_nbest(**kw)["tags"].shape[1] == 4      # args.nbest absent: 4
    m.args.nbest = 2
    assert m.predict_nbest(**kw)["tags"].shape[1] == 2


def test_predict_nbest_ranks_without_a_path_have_no_entities(monkeypatch):
    """The tiny model over a two-label list (PAD, O, B-POS: C = 3), nbest = 8: a three-token sentence has 27 paths, the one-token
    sentences three -- their ranks 3 .. 7 hold no tags, no score and no entity."""
    monkeypatch.setattr(T, "LABELS", ["O", "B-POS"])
    cfg, m = T.tiny_model(False, max_entities=4)
    B, S = 3, 8
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, 53, B, S, lo_id=5))
    mask = torch.zeros_like(mask)
    mask[:, 0] = 1
    mask[0, :3] = 1
    res = m.predict_nbest(input_ids=ids, attention_mask=mask, token_type_ids=tt, nbest=8)
    assert res["n_paths"].tolist() == [8, 3, 3] and tuple(res["entities"].shape) == (B, 8, 4, 3)
    assert bool((res["count"][1:, 3:] == 0).all()) and bool((res["entities"][1:, 3:] == -1).all())
    assert bool((res["confidence"][1:, 3:] == 0).all()) and bool((res["tags"][1:, 3:] == -1).all())
    assert bool(torch.isinf(res["scores"][1:, 3:]).all()) and bool(torch.isinf(res["logprob"][1:, 3:]).all())
    assert sorted(res["tags"][1, :3, 0].tolist()) == [0, 1, 2] and bool((res["tags"][0, :, :3] >= 0).all())
    assert bool(torch.isfinite(res["scores"][0]).all()) and res["lengths"].tolist() == [[3] * 8, [1] * 8, [1] * 8]
