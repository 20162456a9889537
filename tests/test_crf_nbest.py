"""n-best Viterbi without a GPU: the float64 references of tests/crf_nbest_cases.py against each other and against the one-best
oracle, the gap of every listed gapped seed, the tie order, and the shape checks of mtvaf_crf_nbest, which answer before any
launch."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import crf_nbest_cases as N
from mtvaf_amd.hip import crf_nbest  # (the binding this file is about: absent, nothing below has a subject)
from oracle import mtvaf_oracle as O

SMALL = [c for c in N.CASES + N.GAPPED if c[0] ** c[1] <= 4096]


def ident(c):
    return "C{}-S{}-K{}-B{}-seed{}".format(*c)


@pytest.mark.parametrize("case", SMALL, ids=ident)
def test_dp_equals_brute_force(case):
    ref = N.reference(case)
    for b, s in enumerate(ref.sents):
        if case[0] ** s.n > 4096:
            continue
        sc, paths = N.brute(ref.em[b, :s.n], ref.start, ref.end, ref.trans, case[2] + 1)
        assert len(sc) == len(s.scores_ext) == min(case[2] + 1, case[0] ** s.n)
        assert np.abs(sc - s.scores_ext).max() <= 1e-12 * max(1.0, np.abs(sc).max())
        if case in N.GAPPED:
            assert paths[:s.n_paths] == s.paths


@pytest.mark.parametrize("case", N.CASES + N.GAPPED, ids=ident)
def test_references_are_consistent(case):
    """Scores non-increasing, every path's own score is its reported score, paths distinct, and rank 0 is the float64 one-best
    Viterbi (the K = 1 programme too)."""
    ref = N.reference(case)
    inp = ref.inp
    want = O.crf_decode(inp.em.double(), inp.mask, inp.start.double(), inp.end.double(), inp.trans.double())
    for b, s in enumerate(ref.sents):
        assert (np.diff(s.scores_ext) <= 0).all() and len(s.paths) == s.n_paths == min(case[2], case[0] ** s.n)
        for sc, p in zip(s.scores, s.paths):
            assert len(p) == s.n and abs(N.path_score(ref.em[b], ref.start, ref.end, ref.trans, p) - sc) <= 1e-12 * max(1.0, abs(sc))
        assert len({tuple(p) for p in s.paths}) == s.n_paths
        sc1, p1 = N.kbest(ref.em[b, :s.n], ref.start, ref.end, ref.trans, 1)
        assert p1[0] == s.paths[0] and sc1[0] == s.scores[0]
        wsc = N.path_score(ref.em[b], ref.start, ref.end, ref.trans, want[b])
        assert want[b] == s.paths[0] or abs(wsc - s.scores[0]) <= 1e-12 * max(1.0, abs(wsc))
        assert s.logz >= s.scores[0] - 1e-9 and np.exp(s.scores - s.logz).sum() <= 1 + 1e-9


@pytest.mark.parametrize("case", N.GAPPED, ids=ident)
def test_every_gapped_seed_is_gapped(case):
    q = N.min_gap_ratio(N.reference(case))
    print(f"crf-nbest gap {ident(case)}: min gap / delta = {q:.1f}")
    assert q > N.GAP_FACTOR


def test_gapped_cases_cover_every_shape_but_the_long_one():
    shapes = {(C, S, K, B) for C, S, K in N.SHAPES for B in N.BATCHES}
    multi = {(C, S, K, B) for C, S, K in N.MULTI_STAGE for B in N.BATCHES}
    assert {c[:4] for c in N.CASES} == shapes | multi and {c[:4] for c in N.GAPPED} == {s for s in shapes if s[:3] != N.LONG}


def test_the_multi_stage_shapes_cross_a_stage_boundary_of_the_backtrace_and_the_others_do_not():
    stages = lambda C, S, K: -(-(S - 1) // (N.BACKTRACE_STAGE // (K * C)))  # full length: S - 1 back-steps
    assert [stages(*s) for s in N.MULTI_STAGE] == [2, 3] and all(stages(*s) <= 1 for s in N.SHAPES)
    for case in N.CASES:
        if case[:3] in N.MULTI_STAGE:
            assert N.reference(case).sents[0].n == case[1]  # sentence 0 is full length in every batch


def test_tie_case_order():
    inp = N.tie_inputs()
    em, start, end, trans = (x.double().numpy() for x in (inp.em, inp.start, inp.end, inp.trans))
    sc, paths = N.kbest(em[0, :2], start, end, trans, 9)
    assert paths == N.TIE_ORDER and (sc == 0).all()
    assert N.kbest(em[0, :2], start, end, trans, 8)[1] == N.TIE_ORDER[:8]


def test_symbols_declared_exported_and_built():
    from mtvaf_amd import hip
    from mtvaf_amd.build import SOURCES, build_library
    res, _, args = abi_header.prototype("mtvaf_crf_nbest")
    assert res == "int" and ("int32_t*", "n_paths_out") in args
    assert abi_header.prototype("mtvaf_crf_nbest_workspace_bytes") == (
        "size_t", "mtvaf_crf_nbest_workspace_bytes", [("int", "B"), ("int", "S"), ("int", "C"), ("int", "K")])
    assert len(args) == len(hip._SIGS["mtvaf_crf_nbest"][1]) == 16
    assert {"mtvaf_crf_nbest", "mtvaf_crf_nbest_workspace_bytes"} <= set(hip.exported_symbols())
    assert "crf_nbest.hip" in SOURCES
    lib = ctypes.CDLL(build_library(verbose=False))
    assert hasattr(lib, "mtvaf_crf_nbest") and hasattr(lib, "mtvaf_crf_nbest_workspace_bytes")


def workspace_formula(B, S, C, K):
    from mtvaf_amd import hip
    r256 = lambda n: (n + 255) // 256 * 256
    return r256(2 * B * S * K * C) + r256(4 * B) + hip.lib().mtvaf_crf_workspace_bytes(B, S, C)


@pytest.mark.parametrize("B,S,C,K", [(1, 1, 1, 1), (5, 17, 13, 4), (3, 512, 64, 8), (32, 128, 16, 8), (2, 9, 17, 3)])
def test_workspace_query_follows_the_documented_formula(B, S, C, K):
    from mtvaf_amd import hip
    assert hip.lib().mtvaf_crf_nbest_workspace_bytes(B, S, C, K) == workspace_formula(B, S, C, K) > 0


@pytest.mark.parametrize("S,C,K", [(16, 13, 0), (16, 13, 9), (16, 65, 4), (513, 13, 4), (0, 13, 4), (16, 0, 4)])
def test_limits_are_checked_before_any_launch(S, C, K):
    """The library answers its shape status without touching the device (every pointer is NULL); the query returns 0; the Python
    layer raises ValueError."""
    from mtvaf_amd import hip
    assert hip.lib().mtvaf_crf_nbest_workspace_bytes(2, S, C, K) == 0
    assert hip.lib().mtvaf_crf_nbest(None, None, None, None, None, K, None, None, None, None, 2, S, C, None, 1 << 30, None) == -1
    if S > 0 and C > 0:
        with pytest.raises(ValueError):
            crf_nbest(torch.zeros(2, S, C), torch.ones(2, S, dtype=torch.uint8), torch.zeros(C), torch.zeros(C), torch.zeros(C, C), K)


def test_a_short_workspace_is_refused_before_any_launch():
    from mtvaf_amd import hip
    need = hip.lib().mtvaf_crf_nbest_workspace_bytes(2, 16, 13, 4)
    call = lambda wsb: hip.lib().mtvaf_crf_nbest(None, None, None, None, None, 4, None, None, None, None, 2, 16, 13, None, wsb, None)
    assert call(need - 1) == -4 and call(0) == -4
    assert hip.lib().mtvaf_crf_nbest(None, None, None, None, None, 4, None, None, None, None, 0, 16, 13, None, need, None) == -1


def test_python_checks_raise_before_the_library_is_called():
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError):
        crf_nbest(z(2, 8), torch.ones(2, 8, dtype=torch.uint8), z(3), z(3), z(3, 3), 4)
    with pytest.raises(ValueError):
        crf_nbest(z(2, 8, 3), torch.ones(2, 7, dtype=torch.uint8), z(3), z(3), z(3, 3), 4)
    with pytest.raises(ValueError):
        crf_nbest(z(2, 8, 3), torch.ones(2, 8, dtype=torch.uint8), z(4), z(3), z(3, 3), 4)


def test_nbest_to_lists():
    from mtvaf_amd.metrics import nbest_to_lists
    res = {"tags": torch.tensor([[[1, 2, -1], [0, 2, -1]], [[2, -1, -1], [-1, -1, -1]]], dtype=torch.int32),
           "scores": torch.tensor([[3.0, 1.0], [0.5, float("-inf")]]), "n_paths": torch.tensor([2, 1], dtype=torch.int32),
           "logprob": torch.log(torch.tensor([[0.5, 0.25], [1.0, 0.0]]))}
    got = nbest_to_lists(res)
    assert [[h[:2] for h in sent] for sent in got] == [[([1, 2], 3.0), ([0, 2], 1.0)], [([2], 0.5)]]
    assert [h[2] for sent in got for h in sent] == pytest.approx([0.5, 0.25, 1.0], rel=1e-6)
    assert nbest_to_lists(dict(res, logprob=None)) == [[([1, 2], 3.0, None), ([0, 2], 1.0, None)], [([2], 0.5, None)]]


def test_module_surface():
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    from mtvaf_amd.modules.crf import CRF
    assert callable(CRF.decode_nbest) and callable(TVNetSAModel2.predict_nbest)
    import inspect
    sig = inspect.signature(CRF.decode_nbest)
    assert sig.parameters["nbest"].default == 4 and sig.parameters["return_logprob"].default is True
    assert inspect.signature(TVNetSAModel2.predict_nbest).parameters["nbest"].default is None
