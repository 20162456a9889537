"""Inputs, float64 references and bounds shared by the posterior-sampling and minimum-risk tests (test_crf_sample.py on the CPU,
test_crf_sample_gpu.py on the GPU).  Helpers only: no tests, no GPU.

The draw rule (mtvaf_crf_sample), restated in numpy float64 on the float32 inputs: with alpha_t the log forward variables,
    x_i = alpha_t[i] + (t == len-1 ? end[i] : trans[i][y_{t+1}]),  w_i = exp(x_i - max x),  F_j = sum_{i <= j} w_i,
the tag at column t is the smallest j with F_j > u * F_{C-1}; without one, the highest j with w_j > 0.

Inputs are those of crf_nbest_cases.inputs with one change: a constant of the case (``centre``, a multiple of 1/16, the mean growth of
the log-partition per transition of sentence 0; 0 where S = 1) is subtracted from every emission.  A constant per column moves no probability; it
keeps |alpha| of the order of its fluctuation instead of growing by about log C + 2 per column, and the gap below is
proportional to max|alpha|: with alpha near 2500 at column 512 of 64 tags no uniform in [0, 1) would have a gap at all.

Gapped uniforms: a float32 rounding of alpha can move a boundary F_j / F_{C-1} of a draw.  For each draw
    gamma = 2 delta_alpha + C 2^-23,   delta_alpha = 2^-24 (2 len + 1) max|alpha|
(max over the sentence's columns and tags; the form of crf_nbest_cases.delta, the bound the suite holds the recursions to; a
boundary moves by at most the change of the x_i, which alpha and the transition each enter once: twice delta_alpha; C 2^-23 is
the float32 summation of C weights <= 1).  A float32 uniform of the case's generator is kept only if it lies at least 4 gamma
from every interior boundary (the factor 4: the fp32 summation order of the partial sums); otherwise the next value is taken;
more than 64 redraws for one draw fail the case.  Every draw of every case is compared: the returned tags must equal the
reference's.
"""
import functools
import itertools
import types

import numpy as np
import torch

import crf_llh_cases as L
import crf_nbest_cases as N
from oracle import mtvaf_oracle as O

# (C, S, K, B): C at the 16 / 17 edge of the two kernel families, S across one wave and across 128, K = 1 / odd / 64, one case
# at the top of every limit
SHAPES = [(1, 1, 1, 1), (2, 1, 5, 1), (3, 4, 64, 5), (13, 16, 8, 5), (16, 17, 5, 1), (17, 17, 5, 5), (33, 65, 8, 1),
          (64, 5, 64, 5), (13, 130, 8, 5), (64, 512, 2, 1)]
CASES = [(C, S, K, B, 100 * C + S + B) for C, S, K, B in SHAPES]
MRT_CASES = [c for c in CASES if c[:4] in ((13, 16, 8, 5), (17, 17, 5, 5))]
GAP_FACTOR = 4.0
MAX_REDRAWS = 64


def log_alphas(em, start, trans):
    """float64 log forward variables of one sentence: em [len,C] -> [len,C]"""
    a = np.empty_like(em)
    a[0] = start + em[0]
    for t in range(1, em.shape[0]):
        x = a[t - 1][:, None] + trans
        m = x.max(0)
        a[t] = m + np.log(np.exp(x - m).sum(0)) + em[t]
    return a


def inputs(case):
    """crf_nbest_cases.inputs(case) with ``centre`` subtracted from the emissions (module docstring); float32 torch."""
    inp = N.inputs(case)
    em, start, end, trans = (x.double().numpy() for x in (inp.em, inp.start, inp.end, inp.trans))
    n = inp.lengths[0]
    centre = 0.0
    if n > 1:  # (a sentence of one column has nothing that grows)
        growth = N.log_partition(em[0, :n], start, end, trans) - N.log_partition(em[0, :1], start, end, trans)
        centre = round(growth / (n - 1) * 16.0) / 16.0
    inp.em = inp.em - centre  # (exact or not, the float32 result IS the input)
    inp.centre = centre
    return inp


def weights(x):
    return np.exp(x - x.max())


def draw(x, u):
    """the draw rule on one column: x [C] float64, u a float -> tag"""
    w = weights(x)
    F = np.cumsum(w)
    hit = np.nonzero(F > u * F[-1])[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])


def column(alpha, end, trans, t, y_next):
    return alpha[t] + (end if t == alpha.shape[0] - 1 else trans[:, y_next])


def reference_sample(em, start, end, trans, u):
    """One sample of one sentence: em [len,C] float64, u [len] -> tags [len] (the rule above, float64)."""
    alpha = log_alphas(em, start, trans)
    n = em.shape[0]
    y = np.zeros(n, dtype=np.int64)
    for t in range(n - 1, -1, -1):
        y[t] = draw(column(alpha, end, trans, t, y[t + 1] if t + 1 < n else 0), float(u[t]))
    return y


def gamma(n, C, alpha):
    return 2.0 * (2.0 ** -24 * (2 * n + 1) * float(np.abs(alpha).max())) + C * 2.0 ** -23


def make_reference(case):
    """Gapped uniforms [B,K,S] float32 (0 behind the length), the reference tags [B,K,S] (-1 behind it), float64 path scores
    [B,K], logZ [B], per-sentence delta (crf_nbest_cases.delta over the sentence's K scores), the batch's log-partition bound."""
    C, S, K, B, seed = case
    inp = inputs(case)
    em, start, end, trans = (x.double().numpy() for x in (inp.em, inp.start, inp.end, inp.trans))
    gnr = torch.Generator().manual_seed(seed + 7)
    u = np.zeros((B, K, S), dtype=np.float32)
    tags = np.full((B, K, S), -1, dtype=np.int64)
    scores = np.zeros((B, K))
    redraws = 0
    for b, n in enumerate(inp.lengths):
        alpha = log_alphas(em[b, :n], start, trans)
        g = GAP_FACTOR * gamma(n, C, alpha)
        for k in range(K):
            for t in range(n - 1, -1, -1):
                w = weights(column(alpha, end, trans, t, tags[b, k, t + 1] if t + 1 < n else 0))
                F = np.cumsum(w)
                edges = F[:-1] / F[-1]  # the interior boundaries
                for tries in range(MAX_REDRAWS + 1):
                    v = float(torch.rand((), generator=gnr))
                    if not len(edges) or np.abs(edges - v).min() >= g:
                        break
                else:
                    raise AssertionError(f"case {case}: no gapped uniform for sentence {b} sample {k} column {t} after "
                                         f"{MAX_REDRAWS} redraws (4 gamma = {g:.3e})")
                redraws += tries
                u[b, k, t] = v
                hit = np.nonzero(F > v * F[-1])[0]
                tags[b, k, t] = int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])
            scores[b, k] = N.path_score(em[b, :n], start, end, trans, tags[b, k, :n])
    logz = np.array([N.log_partition(em[b, :n], start, end, trans) for b, n in enumerate(inp.lengths)])
    delta = np.array([N.delta(n, scores[b]) for b, n in enumerate(inp.lengths)])
    args64 = (inp.em.double(), inp.mask, inp.start.double(), inp.end.double(), inp.trans.double())
    args32 = (inp.em, inp.mask, inp.start, inp.end, inp.trans)
    z64, z32 = O.crf_log_partition(*args64), O.crf_log_partition(*args32)
    return types.SimpleNamespace(inp=inp, u=torch.from_numpy(u), tags=tags, scores=scores, logz=logz, delta=delta,
                                 logz_bound=L.bound("logz", z64, z32), redraws=redraws, em=em, start=start, end=end, trans=trans)


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs, gapped uniforms and references of ``case``: computed once, shared, not to be modified."""
    return make_reference(case)


# ---- brute force -----------------------------------------------------------------------------------------------------------
def all_paths(em, start, end, trans):
    """-> (paths [C^len, len], probabilities [C^len]) of one sentence, every path enumerated (C^len <= 4096), float64"""
    n, C = em.shape
    assert C ** n <= 4096
    paths = np.array(list(itertools.product(range(C), repeat=n)), dtype=np.int64)
    sc = start[paths[:, 0]] + em[0, paths[:, 0]]
    for t in range(1, n):
        sc = sc + (trans[paths[:, t - 1], paths[:, t]] + em[t, paths[:, t]])
    sc = sc + end[paths[:, -1]]
    p = np.exp(sc - sc.max())
    return paths, p / p.sum(), sc


# ---- minimum risk ----------------------------------------------------------------------------------------------------------
def minimum_risk(em, start, end, trans, mask, hyp, cost, alpha=1.0):
    """The loss of CRF.minimum_risk in the dtype of ``em`` with autograd: em [B,S,C], hyp int64 [B,K,S] (a row is valid iff its
    first column is >= 0; a row equal to an earlier valid row over the unmasked columns is dropped), cost [B,K] -> risk [B]."""
    B, K, S = hyp.shape
    C = em.shape[2]
    on = mask.bool()
    valid = hyp[:, :, 0] >= 0
    for b in range(B):
        seen = []
        for k in range(K):
            row = tuple(hyp[b, k][on[b]].tolist())
            if bool(valid[b, k]) and row in seen:
                valid[b, k] = False
            elif bool(valid[b, k]):
                seen.append(row)
    rows = em[:, None].expand(B, K, S, C).reshape(B * K, S, C)
    llh = O.crf_log_likelihood(rows, hyp.clamp(min=0).reshape(B * K, S), mask[:, None].expand(B, K, S).reshape(B * K, S), start, end,
                               trans, "none").view(B, K)
    risk = []
    for b in range(B):
        if not bool(valid[b].any()):
            risk.append(em.sum() * 0.0)
            continue
        q = torch.softmax(alpha * llh[b][valid[b]], 0)
        risk.append((q * cost[b][valid[b]].to(q.dtype)).sum())
    return torch.stack(risk), llh


def mrt_inputs(case):
    """Hypotheses and costs for the minimum-risk tests of ``case``: the gapped reference samples (so duplicates occur as they
    fall), cost U[0,1) float32 [B,K]."""
    ref = reference(case)
    C, S, K, B, seed = case
    hyp = torch.from_numpy(ref.tags.copy())
    cost = torch.rand(B, K, generator=torch.Generator().manual_seed(seed + 13))
    return ref.inp, hyp, cost


def mrt_oracle(case, alpha, dtype, hyp=None, cost=None):
    """risk [B], the llh of the B * K rows and the gradients of risk.sum() from the oracle in ``dtype``"""
    inp, h, c = mrt_inputs(case)
    hyp, cost = (h if hyp is None else hyp), (c if cost is None else cost)
    em, s, e, t = (x.to(dtype).clone().requires_grad_(True) for x in (inp.em, inp.start, inp.end, inp.trans))
    risk, llh = minimum_risk(em, s, e, t, inp.mask, hyp.clone(), cost, alpha)
    grads = torch.autograd.grad(risk.sum(), [em, s, e, t], allow_unused=True)
    dem, dstart, dend, dtrans = (torch.zeros_like(p) if g is None else g for g, p in zip(grads, (em, s, e, t)))
    return dict(risk=risk.detach(), llh=llh.detach(), dem=dem, dstart=dstart, dend=dend, dtrans=dtrans)


@functools.lru_cache(maxsize=None)
def mrt_reference(case, alpha=1.0):
    r64, r32 = mrt_oracle(case, alpha, torch.float64), mrt_oracle(case, alpha, torch.float32)
    z64 = O.crf_log_partition(*(x.double() if x.dtype.is_floating_point else x for x in
                                (reference(case).inp.em, reference(case).inp.mask, reference(case).inp.start,
                                 reference(case).inp.end, reference(case).inp.trans)))
    bound = {k: L.bound(k, r64[k], r32[k], z64) for k in ("llh", "dem", "dstart", "dend", "dtrans")}
    return types.SimpleNamespace(r64=r64, r32=r32, bound=bound)
