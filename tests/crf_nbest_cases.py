"""Inputs, float64 references and bounds shared by the n-best Viterbi tests (test_crf_nbest.py on the CPU, test_crf_nbest_gpu.py on
the GPU).  Helpers only: no tests, no GPU.

References, numpy float64 on the float32 inputs (exactly representable):
  * ``brute``: all C^len paths enumerated and sorted by score (C^len <= 4096);
  * ``kbest``: the K-best dynamic programme with the tie rule of mtvaf_crf_nbest -- for tag j at step t the K best of
    best[t-1][i][r] + trans[i][j] + em[t][j], equal scores to the lower previous tag, then the lower previous rank; at the end the K
    best of best[len-1][i][r] + end[i], equal scores to the lower last tag, then the lower rank.

Bound of a path score: delta = 2^-24 * (2 len + 1) * max|score|, max over the reference scores of the sentence's returned ranks.  A
path score is 2 len float32 additions whose partial sums stay within that magnitude for these inputs, each rounding at most 2^-24 of
its result; tests/crf_wide_cases.py bounds path scores the same way.  The log-probability adds the bound of the log-partition of
tests/crf_llh_cases.py (``bound("logz", ...)``: the float32 oracle's own error, with a floor of 2e-5 * max|logZ|).

Gapped cases: seeds picked on the CPU (``find_gapped_seed``) so that, in every sentence, consecutive reference scores among ranks
0 .. min(K, n_paths) -- rank K is one past the last one returned -- differ by more than 8 delta: float32 cannot reorder them, so the
returned tags must equal the reference's.  The list is fixed; test_crf_nbest.py asserts the gap for every entry.
"""
import functools
import itertools
import types

import numpy as np
import torch

import crf_llh_cases as L
from oracle import mtvaf_oracle as O

# (C, S, K): the lane boundaries at 16 / 17, 32 / 33 and 64, S = 1, more ranks than paths ((2,1,8): 2 paths, (3,2,8): 9 > 8 of
# them but 3 after the first step), a sentence longer than one wave's worth of steps
SHAPES = [(2, 1, 8), (3, 2, 8), (3, 4, 8), (5, 7, 4), (13, 16, 8), (16, 17, 4), (17, 17, 4), (33, 9, 8), (64, 5, 8), (13, 130, 4)]
# the backtrace stages 8192 // (K * C) steps of back-pointers at a time: these take 2 and 3 stages at full length (78 steps per
# stage against 129, 16 against 39), so tag and rank are carried across a stage boundary; no other shape above leaves one stage
MULTI_STAGE = [(13, 130, 8), (64, 40, 8)]
BACKTRACE_STAGE = 8192
BATCHES = (1, 5)
CASES = [(C, S, K, B, 100 * C + S + B) for C, S, K in SHAPES + MULTI_STAGE for B in BATCHES]
# (C, S, K, B, seed): seeds from find_gapped_seed(C, S, K, B), the first gapped one from 0 upwards.  Every shape but LONG: over 130
# steps the second-best path departs from the best where the two leading tags of a step are closest, a gap of the order of
# (spread of a step) / 130, which is the size of delta itself -- the best of 6000 seeds reaches 3.2 delta at B = 1, none 8 delta.
LONG = (13, 130, 4)
GAPPED = [(2, 1, 8, 1, 0), (2, 1, 8, 5, 0), (3, 2, 8, 1, 0), (3, 2, 8, 5, 0), (3, 4, 8, 1, 0), (3, 4, 8, 5, 0), (5, 7, 4, 1, 0),
          (5, 7, 4, 5, 0), (13, 16, 8, 1, 0), (13, 16, 8, 5, 1), (16, 17, 4, 1, 0), (16, 17, 4, 5, 0), (17, 17, 4, 1, 0),
          (17, 17, 4, 5, 0), (33, 9, 8, 1, 0), (33, 9, 8, 5, 0), (64, 5, 8, 1, 0), (64, 5, 8, 5, 0)]
GAP_FACTOR = 8.0


def lengths_of(S, B, gnr):
    """Ragged: sentence 0 is full; from two sentences on, sentence 1 has length 1; the rest are drawn from 1 .. S."""
    lens = [S] + [1] * (B > 1) + [int(x) for x in torch.randint(1, S + 1, (max(B - 2, 0),), generator=gnr)]
    return lens[:B]


def inputs(case):
    """-> em [B,S,C] = N(0,1) * 2, mask [B,S] uint8 (prefix), start / end [C], trans [C,C] = U(-0.5, 0.5), lengths: float32 torch"""
    C, S, K, B, seed = case
    gnr = torch.Generator().manual_seed(seed)
    em = torch.randn(B, S, C, generator=gnr) * 2
    start, end = torch.rand(C, generator=gnr) - 0.5, torch.rand(C, generator=gnr) - 0.5
    trans = torch.rand(C, C, generator=gnr) - 0.5
    lens = lengths_of(S, B, gnr)
    mask = torch.zeros(B, S, dtype=torch.uint8)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    return types.SimpleNamespace(em=em, mask=mask, start=start, end=end, trans=trans, lengths=lens, K=K)


def tie_inputs():
    """All-zero parameters and emissions, C = 3, one sentence of length 2 (S = 3): nine paths of score 0."""
    return types.SimpleNamespace(em=torch.zeros(1, 3, 3), mask=torch.tensor([[1, 1, 0]], dtype=torch.uint8), start=torch.zeros(3),
                                 end=torch.zeros(3), trans=torch.zeros(3, 3), lengths=[2], K=8)


# the order the tie rule gives: the last tag ascending, under it the previous tag ascending
TIE_ORDER = [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1], [0, 2], [1, 2], [2, 2]]


def path_score(em, start, end, trans, path):
    """float64 score of one path of one sentence: em [len,C] and parameters float64 numpy"""
    s = start[path[0]] + em[0, path[0]]
    for t in range(1, len(path)):
        s += trans[path[t - 1], path[t]] + em[t, path[t]]
    return float(s + end[path[-1]])


def brute(em, start, end, trans, K):
    """-> (scores [min(K, C^len)] non-increasing, paths): every path enumerated"""
    n, C = em.shape
    assert C ** n <= 4096
    paths = np.array(list(itertools.product(range(C), repeat=n)), dtype=np.int64)
    sc = start[paths[:, 0]] + em[0, paths[:, 0]]
    for t in range(1, n):
        sc = sc + (trans[paths[:, t - 1], paths[:, t]] + em[t, paths[:, t]])
    sc = sc + end[paths[:, -1]]
    order = np.argsort(-sc, kind="stable")[:K]
    return sc[order], [paths[o].tolist() for o in order]


def kbest(em, start, end, trans, K):
    """-> (scores [min(K, C^len)] non-increasing, paths): the K-best dynamic programme with the tie rule"""
    n, C = em.shape
    best = np.full((C, K), -np.inf)
    best[:, 0] = start + em[0]
    back = []
    for t in range(1, n):
        cand = (best[:, :, None] + trans[:, None, :]).reshape(C * K, C) + em[t][None, :]  # row i * K + r, column j
        order = np.argsort(-cand, axis=0, kind="stable")[:K]                              # equal scores: the lower (i, r) first
        best = np.take_along_axis(cand, order, axis=0).T.copy()
        back.append(order.T.copy())                                                       # [j][rank] -> i * K + r
    fin = (best + end[:, None]).reshape(C * K)
    order = [o for o in np.argsort(-fin, kind="stable")[:K] if np.isfinite(fin[o])]
    paths = []
    for o in order:
        j, r = divmod(int(o), K)
        p = [j]
        for bk in reversed(back):
            j, r = divmod(int(bk[j, r]), K)
            p.append(j)
        paths.append(p[::-1])
    return fin[order], paths


def log_partition(em, start, end, trans):
    a = start + em[0]
    for t in range(1, em.shape[0]):
        x = a[:, None] + trans
        m = x.max(0)
        a = m + np.log(np.exp(x - m).sum(0)) + em[t]
    a = a + end
    return float(a.max() + np.log(np.exp(a - a.max()).sum()))


def delta(n, scores):
    return 2.0 ** -24 * (2 * n + 1) * float(np.abs(scores).max())


def make_reference(inp):
    """Per sentence: K + 1 reference ranks (the extra one for the gap), logZ, delta; the batch's log-partition bound."""
    em, start, end, trans = (x.double().numpy() for x in (inp.em, inp.start, inp.end, inp.trans))
    C, K = em.shape[2], inp.K
    sents = []
    for b, n in enumerate(inp.lengths):
        sc, paths = kbest(em[b, :n], start, end, trans, K + 1)
        n_paths = min(K, C ** n)
        sents.append(types.SimpleNamespace(n=n, n_paths=n_paths, scores=sc[:n_paths], paths=paths[:n_paths], scores_ext=sc,
                                           logz=log_partition(em[b, :n], start, end, trans), delta=delta(n, sc[:n_paths])))
    args64 = (inp.em.double(), inp.mask, inp.start.double(), inp.end.double(), inp.trans.double())
    args32 = (inp.em, inp.mask, inp.start, inp.end, inp.trans)
    z64, z32 = O.crf_log_partition(*args64), O.crf_log_partition(*args32)
    return types.SimpleNamespace(inp=inp, sents=sents, em=em, start=start, end=end, trans=trans,
                                 logz_bound=L.bound("logz", z64, z32))


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and references of ``case``: computed once, shared, not to be modified."""
    return make_reference(inputs(case))


def min_gap_ratio(ref):
    """min over sentences and consecutive reference ranks 0 .. min(K, n_paths) of (score gap) / delta; inf without a pair"""
    q = np.inf
    for s in ref.sents:
        ext = s.scores_ext[:s.n_paths + 1]
        if len(ext) > 1:
            q = min(q, float((ext[:-1] - ext[1:]).min()) / s.delta)
    return q


def find_gapped_seed(C, S, K, B, limit=2000):
    """The first seed whose case is gapped (how GAPPED was made)."""
    for seed in range(limit):
        if min_gap_ratio(make_reference(inputs((C, S, K, B, seed)))) > GAP_FACTOR:
            return seed
    raise LookupError((C, S, K, B))
