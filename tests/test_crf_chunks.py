"""Chunk-event posteriors without a GPU: the numpy recursion of tests/crf_chunks_cases.py against enumeration of all paths, its
structural properties, the references of the GPU cases, and the torch helpers `CRF.entity_chunk_confidence` / `CRF.chunks_above`
on CPU tensors."""
import numpy as np
import pytest
import torch

import crf_chunks_cases as K

MAPS = {1: [{"O": 0}], 2: [{"O": 0, "B-A": 1}], 3: [{"O": 0, "B-A": 1, "I-A": 2}, {"O": 1, "B-A": 2}, {"O": 0, "B-A": 1, "B-B": 2}]}
S = 7
# (L, kept columns or None for columns 1 .. L-1): dense, gaps of one and two columns, column 0 kept, no kept column, one kept column
LAYOUTS = [(7, None), (7, [1, 3, 6]), (6, [0, 1, 2, 5]), (5, []), (4, [2]), (1, None), (1, [0]), (0, None), (7, [0, 3, 4, 6])]


def small_sentence(C, L, kept, seed):
    """-> em [S,C], mask [S], allowed int64 [S], keep [S] or None, start, end, trans: random sets of density 0.6, singletons inside gaps"""
    rng = np.random.default_rng(seed)
    em, start, end, trans = rng.normal(size=(S, C)) * 1.5, rng.normal(size=C), rng.normal(size=C), rng.normal(size=(C, C))
    mask = (np.arange(S) < L).astype(np.uint8)
    keep = None
    if kept is not None:
        keep = np.zeros(S, dtype=np.uint8)
        keep[kept] = 1
    cols = kept if kept is not None else list(range(1, L))
    allowed = np.zeros(S, dtype=np.int64)
    for t in range(S):
        bits = rng.random(C) < 0.6
        if cols and cols[0] < t < cols[-1] and t not in cols:
            bits = np.zeros(C, dtype=bool)
            bits[rng.integers(0, C)] = True
        allowed[t] = sum(1 << j for j in range(C) if bits[j])  # (0: the full set)
    return em, mask, allowed, keep, start, end, trans


def small_cases():
    n = 0
    for C, maps in MAPS.items():
        for lmap in maps:
            for scheme in ("seqeval", "reference"):
                tab = K.tables_of(lmap, scheme)
                for L, kept in LAYOUTS:
                    n += 1
                    yield f"C{C}-{scheme}-L{L}-{kept}", tab, small_sentence(C, L, kept, 100 + n), 1 + n % 3
    for n, (L, kept) in enumerate(LAYOUTS):
        yield f"random tables L{L}-{kept}", K.random_tables(3, 4, 7 + n), small_sentence(3, L, kept, 500 + n), 1 + n % 3


SMALL = list(small_cases())


@pytest.mark.parametrize("name,tab,sent,W", SMALL, ids=[c[0] for c in SMALL])
def test_recursion_equals_enumeration(name, tab, sent, W):
    em, mask, allowed, keep, start, end, trans = sent
    L, sets, kept = K.sentence_view(mask, allowed, keep, tab.C)
    want, logz_b = K.bruteforce(em, L, sets, kept, start, end, trans, tab, W)
    got, logz = K.recursion(em, L, sets, kept, start, end, trans, tab, W, np.float64)
    assert got.shape == want.shape == (S, W, tab.n_types)
    undefined = np.isnan(want)
    assert (got[undefined] == -np.inf).all()
    assert np.allclose(np.exp(got[~undefined]), want[~undefined], rtol=1e-12, atol=0), name
    assert abs(float(logz) - logz_b) <= 1e-12 * max(1.0, abs(logz_b))
    # the float32 run of the same recursion has the same -inf positions
    got32, _ = K.recursion(em, L, sets, kept, start, end, trans, tab, W, np.float32)
    assert got32.dtype == np.float32 and ((got32 == -np.inf) == (got == -np.inf)).all()


def test_the_layouts_cover_what_they_claim():
    gaps = set()
    for L, kept in LAYOUTS:
        cols = kept if kept is not None else list(range(1, L))
        gaps |= {b - a - 1 for a, b in zip(cols, cols[1:])}
    assert {0, 1, 2} <= gaps
    assert any(kept == [] for _, kept in LAYOUTS) and any(kept is not None and len(kept) == 1 for _, kept in LAYOUTS)
    assert {w for *_, w in SMALL} == {1, 2, 3} and {t.C for _, t, *_ in SMALL} == {1, 2, 3}


@pytest.mark.parametrize("scheme", ["seqeval", "reference"])
def test_singleton_sets_give_the_chunks_of_the_path(scheme):
    """Every set a singleton: the chain is one path, an event has probability 1 if the chunker emits it on that path and 0 if not."""
    import crf_entities_cases as X
    lmap = X.label_map(11)
    tab = K.tables_of(lmap, scheme)
    rng, S_, W, seen = np.random.default_rng(5), 24, 24, 0
    for trial in range(8):
        tags = rng.integers(0, 11, S_)
        L = int(rng.integers(1, S_ + 1))
        keep = (rng.random(S_) < 0.7).astype(np.uint8) if trial % 2 else None
        mask = (np.arange(S_) < L).astype(np.uint8)
        allowed = np.array([1 << int(t) for t in tags], dtype=np.int64)
        em, start, end, trans = rng.normal(size=(S_, 11)), rng.normal(size=11), rng.normal(size=11), rng.normal(size=(11, 11))
        Lv, sets, kept = K.sentence_view(mask, allowed, keep, 11)
        got, _ = K.recursion(em, Lv, sets, kept, start, end, trans, tab, W)
        want = {(kept[b], e - b, ty) for ty, b, e in K.table_chunks(tab, [int(tags[c]) for c in kept])}
        finite = {tuple(int(v) for v in idx) for idx in np.argwhere(np.isfinite(got))}
        assert finite == want
        assert all(abs(got[idx]) < 1e-9 for idx in finite) and (got[~np.isfinite(got)] == -np.inf).all()
        seen += len(want)
    assert seen > 10


def test_chunks_that_end_at_one_column_exclude_each_other():
    """With W covering the sentence, the events that end at a kept column e -- over all starts and types -- are disjoint."""
    checked = 0
    for name, tab, sent, _ in SMALL:
        em, mask, allowed, keep, start, end, trans = sent
        L, sets, kept = K.sentence_view(mask, allowed, keep, tab.C)
        if not kept:
            continue
        W = len(kept)
        p = np.exp(K.recursion(em, L, sets, kept, start, end, trans, tab, W)[0])
        for eo in range(len(kept)):
            total = sum(p[kept[bo], eo - bo].sum() for bo in range(eo + 1))
            assert total <= 1 + 1e-12, (name, eo, total)
            checked += 1
    assert checked > 100


def test_the_references_of_the_gpu_cases():
    """Every case has a reference; by the assertion in `make_reference`, at scale 1 at least 99 % of the finite entries lie above
    the floor; the float32 recursion alone meets the acceptance rule; the cases cover the shapes they claim."""
    for case in K.CASES:
        ref = K.reference(case)
        assert ref.defined > 0 or case[1] <= 2, case
        K.check(f"ref32 {K.case_id(case)}", ref, ref.ref32, ref.logz32)
    assert {c[2] for c in K.CASES} == {1, 2, 11, 17, 64} and {c[3] for c in K.CASES} == {1, 2, 8, 16}
    assert {c[:2] for c in K.CASES} == {(1, 1), (5, 2), (9, 17), (5, 65), (9, 130), (1, 512)}
    assert {c[4] for c in K.CASES} == {1, 6} and {c[5] for c in K.CASES} == {"dense", "gaps"} and K.TIE_CASE in K.CASES
    inp = K.reference((9, 130, 17, 16, 1, "gaps")).inp
    lens = K.X.lengths_of(inp.mask)
    assert lens[0] == 130 and lens[1] == 1
    # the gaps family has gaps, and its sets are singletons there
    kept = np.flatnonzero(inp.keep[0].numpy())
    assert (np.diff(kept) > 1).any()
    inner = [c for c in range(kept[0], kept[-1]) if c not in kept]
    assert all(bin(int(inp.allowed[0, c]) & ((1 << 17) - 1)).count("1") == 1 for c in inner)


# ---- the torch helpers -----------------------------------------------------------------------------------------------------
def test_entity_chunk_confidence_is_direct_indexing():
    from mtvaf_amd.modules.crf import CRF
    g = torch.Generator().manual_seed(3)
    B, S_, W, T = 3, 12, 3, 4
    log_post = -torch.rand(B, S_, W, T, generator=g)
    keep = torch.zeros(B, S_, dtype=torch.uint8)
    keep[:, [1, 2, 4, 7, 8, 9]] = 1
    #            (start, end, type): widths 0, 1 (a gap inside), 2, one too wide, one unused slot
    ents = torch.tensor([[[1, 1, 0], [2, 4, 3], [4, 8, 1], [1, 8, 2], [-1, -1, -1]]] * B, dtype=torch.int32)
    got = CRF.entity_chunk_confidence(ents, log_post, keep)
    assert tuple(got.shape) == (B, 5)
    for r in range(B):
        assert got[r, 0] == log_post[r, 1, 0, 0] and got[r, 1] == log_post[r, 2, 1, 3] and got[r, 2] == log_post[r, 4, 2, 1]
        assert got[r, 3] == float("-inf") and got[r, 4] == 0


def test_chunks_above_orders_by_end_then_start_and_pads():
    from mtvaf_amd.modules.crf import CRF
    B, S_, W, T = 2, 10, 3, 2
    log_post = torch.full((B, S_, W, T), float("-inf"))
    keep = torch.zeros(B, S_, dtype=torch.uint8)
    keep[:, [1, 2, 5, 6]] = 1
    lp = {(5, 1, 0): -0.1, (1, 0, 1): -0.2, (1, 2, 0): -0.3, (2, 1, 1): -0.05, (6, 0, 0): -3.0}  # (b, w, T): ends 6, 1, 5, 5, 6
    for (b, w, t), v in lp.items():
        log_post[0, b, w, t] = v
    out = CRF.chunks_above(log_post, keep, threshold=0.5, max_entities=3)
    assert out["count"].tolist() == [4, 0]
    assert out["entities"][0].tolist() == [[1, 1, 1], [1, 5, 0], [2, 5, 1]]           # (1,5) before (2,5): the start breaks the tie
    assert torch.allclose(out["log_confidence"][0], torch.tensor([-0.2, -0.3, -0.05]))
    assert torch.allclose(out["confidence"][0], torch.exp(torch.tensor([-0.2, -0.3, -0.05])))
    assert (out["entities"][1] == -1).all() and (out["confidence"][1] == 0).all() and (out["log_confidence"][1] == 0).all()
    wide = CRF.chunks_above(log_post, keep, threshold=0.01, max_entities=70)
    assert tuple(wide["entities"].shape) == (B, 70, 3) and wide["count"].tolist() == [5, 0]
    assert wide["entities"][0, :5].tolist() == [[1, 1, 1], [1, 5, 0], [2, 5, 1], [5, 6, 0], [6, 6, 0]]
    assert (wide["entities"][0, 5:] == -1).all()
    with pytest.raises(ValueError):
        CRF.chunks_above(log_post, keep, threshold=0.0)


def test_the_binding_declares_the_entry_point():
    from mtvaf_amd import hip
    assert {"mtvaf_crf_chunk_posteriors", "mtvaf_crf_chunk_posteriors_workspace_bytes"} <= set(hip.exported_symbols())
    lib = hip.lib()
    assert lib.mtvaf_crf_chunk_posteriors_workspace_bytes(2, 3, 4) == 2 * 2 * 3 * 64 * 4
    assert lib.mtvaf_crf_chunk_posteriors_workspace_bytes(2, 513, 4) == 0
    # bad sizes and a short workspace are refused before anything is launched (no device is touched)
    def rc(S=3, C=4, n_types=2, W=2, wsb=1 << 20, ws=8):
        return lib.mtvaf_crf_chunk_posteriors(None, None, None, None, None, None, None, None, None, None, n_types, W, None, None,
                                              2, S, C, ws, wsb, None)
    assert rc(S=513) == -1 and rc(C=65) == -1 and rc(S=0) == -1
    assert rc(n_types=0) == -3 and rc(n_types=65) == -3 and rc(W=0) == -3 and rc(W=17) == -3
    assert rc(wsb=100) == -4 and rc(ws=None) == -4
