"""Chunk-event posteriors on the MI355X: `mtvaf_crf_chunk_posteriors` / `CRF.chunk_posteriors` / `TVNetSAModel2.predict_posteriors`
against the float64 recursion of tests/crf_chunks_cases.py (itself pinned against enumeration in test_crf_chunks.py) under the
likelihood rule, -inf positions exactly; ties to the merged kernels; determinism, full overwrite, graph replay; the model.
err / bound is printed per case and asserted <= 1 (the largest per family is recorded in DESIGN.md section 4.13)."""
import numpy as np
import pytest
import torch

import crf_chunks_cases as K
import crf_entities_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_crf(start, end, trans):
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(start.numel(), batch_first=True).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start)
        crf.end_transitions.copy_(end)
        crf.transitions.copy_(trans)
    return crf


def device_tables(tab):
    from mtvaf_amd.metrics import entity_device_tables
    return entity_device_tables(tab.full, DEV)


def run(inp, **kw):
    crf = make_crf(inp.start, inp.end, inp.trans)
    args = dict(keep=None if inp.keep is None else inp.keep.to(DEV), allowed=None if inp.allowed is None else inp.allowed.to(DEV),
                max_width=inp.W)
    args.update(kw)
    return crf, crf.chunk_posteriors(inp.em.to(DEV), inp.mask.to(DEV), device_tables(inp.tab), **args)


# ---- 1. the kernel against the recursion -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_against_the_float64_recursion(case):
    ref = K.reference(case)
    _, (log_post, logz_a) = run(ref.inp, check=True)
    B, S, C, W = case[:4]
    assert tuple(log_post.shape) == (B, S, W, ref.inp.tab.n_types) and tuple(logz_a.shape) == (B,)
    K.check(K.case_id(case), ref, log_post.cpu().numpy(), logz_a.cpu().numpy())


# ---- 2. ties to the merged kernels, (5, 65, 11) ------------------------------------------------------------------------------
def tie_inputs(W=8):
    inp = K.inputs(K.TIE_CASE[:3] + (W,) + K.TIE_CASE[4:])
    return inp, make_crf(inp.start, inp.end, inp.trans), device_tables(inp.tab)


def test_logz_a_is_the_lattice_kernel_s():
    from mtvaf_amd.constraints import structural_sets
    inp, crf, t = tie_inputs()
    allowed = structural_sets(inp.lmap, inp.mask, None)
    inp.allowed = allowed
    ref = K.make_reference(inp)
    em, mask = inp.em.to(DEV), inp.mask.to(DEV)
    _, logz_a = crf.chunk_posteriors(em, mask, t, allowed=allowed.to(DEV), max_width=inp.W)
    _, lat, _ = crf.partial_llh(em, allowed.to(DEV), mask, return_parts=True)
    err = float((logz_a.double() - lat.detach().double()).abs().max())
    print(f"crf-chunks logz_a vs lattice_fwd: err {err:.3e}, bound {ref.bound_logz:.3e}")
    assert err <= ref.bound_logz
    K.check("tie logz_a", ref, crf.chunk_posteriors(em, mask, t, allowed=allowed.to(DEV), max_width=inp.W)[0].cpu().numpy(),
            logz_a.cpu().numpy())


def test_singleton_sets_give_the_chunks_of_crf_entities():
    from mtvaf_amd.constraints import sets_from_labels
    inp, crf, t = tie_inputs(W=16)
    em, mask = inp.em.to(DEV), inp.mask.to(DEV)
    ent = crf.entities(em, mask, t, max_entities=64)  # Viterbi's tags, columns 1 .. L-1
    allowed = sets_from_labels(ent["tags"].clamp(min=0), 11)
    log_post, _ = crf.chunk_posteriors(em, mask, t, allowed=allowed, max_width=16)
    lp = log_post.cpu().numpy()
    assert ((lp == -np.inf) | np.isfinite(lp)).all()
    got = {tuple(int(v) for v in idx) for idx in np.argwhere(np.isfinite(lp))}  # (sentence, start column, width, type)
    e, n = ent["entities"].cpu().numpy(), ent["count"].cpu().numpy()
    assert (n <= 64).all() and n.sum() > 20
    want = {(r, int(e[r, k, 0]), int(e[r, k, 1] - e[r, k, 0]), int(e[r, k, 2])) for r in range(e.shape[0]) for k in range(n[r])
            if e[r, k, 1] - e[r, k, 0] < 16}  # (all columns from 1 are kept: the width is the column difference)
    assert got == want
    bound = 2e-5 * float(crf.partial_llh(em, allowed, mask, return_parts=True)[1].abs().max())
    assert float(np.abs(lp[np.isfinite(lp)]).max()) <= bound  # log 1, up to the rule's projection of logZ_A


def test_single_word_sentences_give_the_constrained_marginal():
    """One kept column: the event (b, 0, T) is "the label there starts and ends a chunk of type T behind / in front of the
    boundary", a sum of node posteriors.  Tolerance: the marginals rule of tests/crf_lattice_cases.py at max|ref| <= 1
    (1e-4 + 1e-7) plus the rule's bound on the log posterior, which is a relative error of a probability <= 1."""
    inp, crf, t = tie_inputs()
    em, mask = inp.em.to(DEV), inp.mask.to(DEV)
    L = X.lengths_of(inp.mask)
    cols = [int(l) // 2 for l in L]  # (L = 1: column 0)
    keep = torch.zeros_like(inp.mask)
    for r, c in enumerate(cols):
        keep[r, c] = 1
    g = torch.Generator().manual_seed(8)
    allowed = torch.where(torch.rand(5, 65, generator=g) < 0.5, torch.randint(1, 1 << 11, (5, 65), generator=g),
                          torch.zeros(5, 65, dtype=torch.int64))  # a random set, or none
    inp.keep, inp.allowed = keep, allowed
    ref = K.make_reference(inp)
    log_post, _ = crf.chunk_posteriors(em, mask, t, keep=keep.to(DEV), allowed=allowed.to(DEV), max_width=inp.W)
    K.check("single word", ref, log_post.cpu().numpy())
    marg = crf.constrained_marginals(em, allowed.to(DEV), mask).cpu().double()
    both = torch.from_numpy(inp.tab.start[11, :11] & inp.tab.end[:11, 11])
    assert bool(both.any())
    err = 0.0
    for r, c in enumerate(cols):
        p = float(torch.exp(log_post[r, c, 0].double()).sum())
        err = max(err, abs(p - float(marg[r, c][both].sum())))
        assert bool((log_post[r, c, 1:] == float("-inf")).all())
    print(f"crf-chunks single word vs constrained_marginals: err {err:.3e}, tolerance {1e-4 + 1e-7 + ref.bound:.3e}")
    assert err <= 1e-4 + 1e-7 + ref.bound


# ---- 3. determinism, full overwrite, capture -----------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_and_every_element_is_written():
    from mtvaf_amd import hip
    for case in [(9, 130, 17, 16, 1, "gaps"), (5, 2, 2, 2, 1, "dense")]:
        inp = K.reference(case).inp
        crf, (first, logz) = run(inp)
        _, (second, logz2) = run(inp)
        assert torch.equal(first, second) and torch.equal(logz, logz2)  # (-inf == -inf; a NaN would not compare equal)
        t = device_tables(inp.tab)
        out = (torch.full_like(first, float("nan")), torch.full_like(logz, float("nan")))
        got = hip.crf_chunk_posteriors(inp.em.to(DEV), None if inp.allowed is None else inp.allowed.to(DEV), inp.mask.to(DEV),
                                       None if inp.keep is None else inp.keep.to(DEV), crf.start_transitions.data,
                                       crf.end_transitions.data, crf.transitions.data, t["start"], t["end"], t["type_of"],
                                       t["n_types"], inp.W, out=out)
        assert got[0] is out[0] and torch.equal(out[0], first) and torch.equal(out[1], logz)


def test_graph_replay_equals_the_eager_call():
    """One capture in a single-stream graph, replayed after the emissions changed in place."""
    inp = K.reference((9, 17, 11, 8, 1, "gaps")).inp
    em2 = K.inputs((9, 17, 11, 8, 6, "gaps")).em
    crf, t = make_crf(inp.start, inp.end, inp.trans), device_tables(inp.tab)
    buf, mask, keep, allowed = inp.em.to(DEV).clone(), inp.mask.to(DEV), inp.keep.to(DEV), inp.allowed.to(DEV)
    crf.chunk_posteriors(buf, mask, t, keep=keep, allowed=allowed, max_width=8)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crf.chunk_posteriors(buf, mask, t, keep=keep, allowed=allowed, max_width=8)
    seen = []
    for emissions in (inp.em, em2):
        buf.copy_(emissions)
        graph.replay()
        torch.cuda.synchronize()
        eager = crf.chunk_posteriors(emissions.to(DEV), mask, t, keep=keep, allowed=allowed, max_width=8)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1])


def test_bad_arguments():
    inp = K.reference((9, 17, 11, 8, 1, "gaps")).inp
    crf, t = make_crf(inp.start, inp.end, inp.trans), device_tables(inp.tab)
    em, mask, keep, allowed = inp.em.to(DEV), inp.mask.to(DEV), inp.keep.to(DEV), inp.allowed.to(DEV)
    for kw in (dict(max_width=0), dict(max_width=17), dict(keep=keep[:, :5]), dict(allowed=allowed.int())):
        with pytest.raises(ValueError):
            crf.chunk_posteriors(em, mask, t, **{**dict(keep=keep, allowed=allowed), **kw})
    # a non-kept column between kept columns that carries more than one tag: outside the contract, reported by check=True only
    crf.chunk_posteriors(em, mask, t, keep=keep, allowed=allowed, check=True)
    with pytest.raises(ValueError):
        crf.chunk_posteriors(em, mask, t, keep=keep, allowed=torch.zeros_like(allowed), check=True)
    log_post, _ = crf.chunk_posteriors(em, mask, t, keep=keep, allowed=torch.zeros_like(allowed))
    assert not bool(torch.isnan(log_post).any())


# ---- 4. the model ------------------------------------------------------------------------------------------------------------
def test_predict_posteriors_on_the_golden_weights():
    import params as P
    import test_model_gpu as M
    from mtvaf_amd.metrics import posteriors_to_lists
    fx = M.load("tvnet2_base_B2S16")
    seed, B, S, n_aux = int(fx["seed"]), int(fx["B"]), int(fx["S"]), int(fx["n_aux"])
    cfg = P.BASE_BERT
    m = M.build_tvnet2(cfg, M.make_args(), sde=P.encoder_params(cfg, seed, std=0.03), sdh=P.head_params(cfg, seed + 10),
                       sdp=P.prompt_params(seed + 20))
    ids, mask, tt, _ = P.text_batch(cfg, seed + 1, B, S, lo_id=1000)
    feats, aux, _ = M._prompt_inputs(seed + 2, B, n_aux)
    kw = dict(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), token_type_ids=tt.to(DEV), images=feats.to(DEV),
              aux_imgs=aux.to(DEV))
    con = m.predict_constrained(**kw)
    res = m.predict_posteriors(threshold=0.51, **kw)
    dec = res["decoded"]
    for k in ("tags", "lengths", "entities", "log_confidence", "confidence", "count"):
        assert torch.equal(dec[k], con[k]), k
    assert dec["types"] == con["types"] == res["types"]
    T = len(res["types"])
    assert tuple(res["log_post"].shape) == (B, S, 8, T) and tuple(dec["chunk_log_conf"].shape) == tuple(dec["confidence"].shape)
    assert float(dec["chunk_log_conf"].max()) <= 1e-6
    used = dec["entities"][..., 0] >= 0
    narrow = used & (dec["entities"][..., 1] - dec["entities"][..., 0] < 8)
    assert bool(torch.isfinite(dec["chunk_log_conf"][narrow]).all())  # a decoded entity is an event the chain can produce
    assert bool((dec["chunk_log_conf"][~used] == 0).all())
    assert float(res["log_post"][torch.isfinite(res["log_post"])].max()) <= 1e-6
    sel = res["selected"]
    e, n = sel["entities"].cpu().numpy(), sel["count"].cpu().numpy()
    for r in range(B):
        spans = [(int(e[r, k, 0]), int(e[r, k, 1])) for k in range(min(int(n[r]), e.shape[1]))]
        assert all(0 < b <= c for b, c in spans)
        assert all(spans[k][1] < spans[k + 1][0] for k in range(len(spans) - 1)), spans  # ordered by end, no overlap
    assert bool((sel["confidence"][sel["entities"][..., 0] >= 0] >= 0.51 - 1e-6).all())
    lists = posteriors_to_lists(res)
    assert len(lists) == B and [len(x["decoded"]) for x in lists] == np.minimum(dec["count"].cpu().numpy(), 32).tolist()
    assert [len(x["selected"]) for x in lists] == np.minimum(n, 32).tolist()
    # max_entity_width and a word mask reach the kernel
    m.args.max_entity_width = 3
    wm = torch.zeros(B, S, dtype=torch.long)
    wm[:, 1::2] = 1
    res3 = m.predict_posteriors(word_mask=wm.to(DEV), **kw)
    assert tuple(res3["log_post"].shape) == (B, S, 3, T)
    assert bool((res3["log_post"][:, 0::2] == float("-inf")).all()) and bool(torch.isfinite(res3["log_post"][:, 1::2]).any())
    con3 = m.predict_constrained(word_mask=wm.to(DEV), **kw)
    assert torch.equal(res3["decoded"]["entities"], con3["entities"])
    assert float(res3["decoded"]["chunk_log_conf"].max()) <= 1e-6
