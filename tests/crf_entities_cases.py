"""Inputs, references and the acceptance rule shared by the tests of `mtvaf_crf_entities` / `CRF.entities` /
`TVNetSAModel2.predict` (test_crf_entities.py on the CPU, test_crf_entities_gpu.py on the GPU).

Reference chunker: `entity_cases.chunks` -- the sequential restatement on label NAMES -- over the kept predicted labels of a
sentence, mapped back to column coordinates; a chunk without a start is dropped.  Kept columns: those below the sentence's
length L (the leading ones of the mask) with ``keep`` set, or columns 1 .. L-1 without a ``keep``.

Reference confidence: the constrained partition function.  Per chunk, `O.crf_log_partition` of the sentence with the emissions
of columns b..e set to -inf everywhere except the decoded tag, minus the unconstrained `O.crf_log_partition`: in float64
(``ref64``) and again in float32 (``ref32``).  All chunks of a case go through the oracle as one batch of copies of their sentences.

Acceptance rule, the one for likelihoods of tests/crf_llh_cases.py: an element passes if
    |got - ref64| <= max(2e-5 * max|logZ64|, 4 * max|ref32 - ref64|)
with both maxima over the case.  The float32 reference alone meets it by construction."""
import types

import numpy as np
import torch

import crf_wide_cases as W
import entity_cases as E
from oracle import mtvaf_oracle as O

SCHEMES = ("seqeval", "reference")

# (B, S, C, scale) as crf_wide_cases.fixed_case reads them.  C: 1 and 2 are the degenerate tag sets (62 / 63 lanes of -inf), 11 /
# 16 / 64 the three label sets, 17 the first width past a 16-lane row; S: 1, 2, around the 64-column ballot word, 130 = three words
# and nine 16-column windows; B: 1, 5, 9 = one wave, a block and one more wave, three blocks with a one-wave tail.
CASES = [(1, 1, 1, 1), (5, 65, 1, 1), (9, 130, 1, 6),
         (5, 2, 2, 1), (9, 64, 2, 6), (1, 130, 2, 1), (3, 16, 2, 1),
         (1, 63, 11, 1), (3, 65, 11, 1), (3, 65, 11, 6), (9, 130, 11, 1),
         (5, 64, 16, 1), (9, 1, 16, 1), (1, 130, 16, 6),
         (5, 63, 17, 1), (1, 2, 17, 6), (9, 65, 17, 1),
         (1, 64, 64, 1), (9, 2, 64, 1), (5, 65, 64, 6), (1, 130, 64, 1)]
# more sentences than the launch has waves (1024 blocks of 4): the grid-stride loop makes a second trip
STRIDE_CASE = (4100, 3, 2, 1)


def label_map(C):
    """A label map with ids 0 .. C-1: the three sets of entity_cases at their widths, cut or extended for the others."""
    if C == 11:
        return E.label_map("a")
    if C == 16:
        return E.label_map("b")
    if C == 64:
        return E.label_map("c")
    if C == 1:
        return {"O": 0}                      # id 0 reads "PAD": under "seqeval" the whole sentence is one chunk of type "AD"
    if C == 2:
        return {"O": 0, "B-POS": 1}
    assert C == 17
    return {n: i for i, n in enumerate(E.SET_B + ["X"], 0)}


def lengths_of(mask):
    """leading ones of every row"""
    m = np.asarray(mask) != 0
    return np.where(m.all(1), m.shape[1], (~m).argmax(1))


def ragged_mask(mask):
    """fixed_case's prefix mask (sentence 0 is full) with L = 1 planted in sentence 1"""
    mask = mask.clone()
    if mask.shape[0] > 1:
        mask[1, 1:] = 0
    return mask


def inputs(case):
    """-> em, random tags, mask, start, end, trans of a (B, S, C, scale) case, the mask ragged with L = S and L = 1 in it"""
    em, tags, mask, start, end, trans = W.fixed_case(*case)
    return em, tags, ragged_mask(mask), start, end, trans


def chunks_of(lmap, scheme, tags, mask, keep=None):
    """-> per sentence [(begin column, end column, type name)], ordered by end column"""
    labs = E.labels_of(lmap)
    C = len(labs)
    tags, out = np.asarray(tags), []
    for r, L in enumerate(lengths_of(mask)):
        cols = [c for c in range(int(L)) if (keep[r][c] if keep is not None else c >= 1)]
        seq = [labs[t if 0 <= t < C else 0] for t in (int(tags[r, c]) for c in cols)]
        out.append([(cols[b], cols[e], ty) for ty, b, e in E.chunks(scheme, seq) if b is not None])
    return out


def sanitised(tags, C):
    t = torch.as_tensor(np.asarray(tags)).long()
    return torch.where((t >= 0) & (t < C), t, torch.zeros_like(t))


def log_posteriors(em, mask, start, end, trans, tags, segments, dtype):
    """log p(y_b..y_e = tags | x) of every (sentence, b, e) in ``segments`` by the constrained partition function, in ``dtype``;
    also the unconstrained logZ [B]."""
    em_, s_, e_, t_ = (x.to(dtype) for x in (em, start, end, trans))
    logz = O.crf_log_partition(em_, mask, s_, e_, t_)
    if not segments:
        return torch.zeros(0, dtype=dtype), logz
    rows = torch.tensor([r for r, _, _ in segments])
    tg = sanitised(tags, em.shape[2])
    con = em_[rows].clone()
    for n, (r, b, e) in enumerate(segments):
        only = torch.full_like(con[n, b:e + 1], float("-inf"))
        cols = torch.arange(b, e + 1)
        only[cols - b, tg[r, cols]] = con[n, cols, tg[r, cols]]
        con[n, b:e + 1] = only
    return O.crf_log_partition(con, mask[rows], s_, e_, t_) - logz[rows], logz


def bound(ref64, ref32, logz64):
    return max(2e-5 * float(logz64.abs().max()), 4.0 * float((ref32.double() - ref64).abs().max()) if len(ref64) else 0.0)


def reference(inp, tags, lmap, keep=None, schemes=SCHEMES, max_entities=64):
    """The expected chunks of every scheme and the reference log posteriors of the segments a call with ``max_entities`` stores (the
    first of every sentence; the union over the schemes goes through the oracle once).
    -> namespace: chunks[scheme], ref64 / ref32 {(r, b, e): value}, logz64, bound."""
    em, _, mask, start, end, trans = inp
    chunks = {s: chunks_of(lmap, s, tags, mask, keep) for s in schemes}
    segments = sorted({(r, b, e) for s in schemes for r, row in enumerate(chunks[s]) for b, e, _ in row[:max_entities]})
    r64, logz64 = log_posteriors(em, mask, start, end, trans, tags, segments, torch.float64)
    r32, _ = log_posteriors(em, mask, start, end, trans, tags, segments, torch.float32)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    return types.SimpleNamespace(chunks=chunks, segments=segments, ref64=dict(zip(segments, r64.tolist())),
                                 ref32=dict(zip(segments, r32.tolist())), logz64=logz64, bound=bound(r64, r32, logz64))


def expected(chunks, types_, max_entities):
    """-> ents [B,E,3] int32 (-1 padded), count [B]: what the kernel must store for these chunks"""
    B = len(chunks)
    ents, count = np.full((B, max_entities, 3), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for r, row in enumerate(chunks):
        count[r] = len(row)
        for k, (b, e, ty) in enumerate(row[:max_entities]):
            ents[r, k] = (b, e, types_.index(ty))
    return ents, count


def ratio(what, ents, log_conf, ref):
    """max |log_conf - ref64| / bound over the stored chunks (0 without any); printed, the tests assert <= 1"""
    err = 0.0
    for r in range(ents.shape[0]):
        for k in range(ents.shape[1]):
            if ents[r, k, 0] >= 0:
                err = max(err, abs(float(log_conf[r, k]) - ref.ref64[(r, int(ents[r, k, 0]), int(ents[r, k, 1]))]))
    q = err / ref.bound if ref.bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"crf-entities ratio {what} {q:.4f} (err {err:.3e}, bound {ref.bound:.3e})")
    return q


def bruteforce_log_posterior(em, mask, start, end, trans, tags, r, b, e):
    """log p(y_b..y_e = tags | x) of sentence r in float64 by enumerating all C^L paths"""
    emd, sd, ed, td = (x.double() for x in (em, start, end, trans))
    C, L = em.shape[2], int(lengths_of(mask)[r])
    paths = torch.cartesian_prod(*[torch.arange(C)] * L).reshape(-1, L)
    sc = sd[paths[:, 0]] + emd[r, 0, paths[:, 0]] + ed[paths[:, -1]]
    for t in range(1, L):
        sc = sc + td[paths[:, t - 1], paths[:, t]] + emd[r, t, paths[:, t]]
    hit = (paths[:, b:e + 1] == torch.as_tensor(tags)[r, b:e + 1].long()[None]).all(1)
    return float(torch.logsumexp(sc[hit], 0) - torch.logsumexp(sc, 0))
