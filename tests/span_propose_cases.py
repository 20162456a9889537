"""Candidate-span proposal: a plain NumPy / Python restatement of the rule `mtvaf_span_propose` implements, and the case table the
GPU tests run it over.  The restatement follows the written rule (include/mtvaf_hip.h), not the kernel: lists,
Python floats (fp64) and the built-in stable sort.

    propose_row(start_logits, end_logits, word_index, word_key, ...)  one sentence  -> (starts, ends, masks, scores, count)
    propose(...)                                                      a batch       -> arrays shaped like the kernel's outputs
"""
from __future__ import annotations

import numpy as np


def signature(word_index, word_key, s, e):
    """Keys of the span's words: word_key[t] wherever word_index[t] differs from the previous in-map token of the span."""
    sig, prev = [], None
    for t in range(s, e + 1):
        if word_index[t] < 0:
            continue
        if prev is None or word_index[t] != prev:
            sig.append(int(word_key[t]))
        prev = word_index[t]
    return tuple(sig)


def propose_row(start_logits, end_logits, word_index, word_key, n_best, max_len, threshold, use_heuristics, nms):
    S = len(start_logits)
    sl = [float(x) for x in start_logits]  # fp32 values as Python floats: every sum below is fp64
    el = [float(x) for x in end_logits]
    thr = float(np.float32(threshold))     # the C ABI carries the threshold as a float
    wk = word_index if word_key is None else word_key
    n = min(n_best, S)
    SI = sorted(range(S), key=lambda p: (-sl[p], p))[:n]
    EI = sorted(range(S), key=lambda p: (-el[p], p))[:n]
    cands = []  # (key, q, s, e)
    for i, s in enumerate(SI):
        for j, e in enumerate(EI):
            if word_index[s] < 0 or word_index[e] < 0 or e < s or e - s + 1 > max_len:
                continue
            total = sl[s] + el[e]
            if not total >= thr:
                continue
            cands.append((total - (e - s + 1) if use_heuristics else total, i * n_best + j, s, e))
    cands.sort(key=lambda c: (-c[0], c[1]))
    starts, ends, scores, sigs, keys = [], [], [], [], set()
    for _, _, s, e in cands:
        if 2 * len(starts) >= n_best:
            break
        sig = signature(word_index, wk, s, e)
        if sig in sigs:
            continue
        if nms == 1 and keys & set(sig):
            continue
        starts.append(s)
        ends.append(e)
        scores.append(np.float32(sl[s] + el[e]))
        sigs.append(sig)
        keys |= set(sig)
    count = len(starts)
    pad = n_best - count
    return starts + [0] * pad, ends + [0] * pad, [1] * count + [0] * pad, scores + [np.float32(0)] * pad, count


def propose(start_logits, end_logits, word_index, word_key, n_best, max_len, threshold, use_heuristics, nms):
    """start_logits / end_logits [B,S] fp32, word_index [B,S] int, word_key [B,S] int or None."""
    B = start_logits.shape[0]
    out = dict(span_starts=np.zeros((B, n_best), np.int64), span_ends=np.zeros((B, n_best), np.int64),
               label_masks=np.zeros((B, n_best), np.int64), span_scores=np.zeros((B, n_best), np.float32),
               count=np.zeros(B, np.int32))
    for b in range(B):
        st, en, ma, sc, c = propose_row(start_logits[b], end_logits[b], word_index[b],
                                        None if word_key is None else word_key[b], n_best, max_len, threshold,
                                        use_heuristics, nms)
        out["span_starts"][b], out["span_ends"][b], out["label_masks"][b] = st, en, ma
        out["span_scores"][b], out["count"][b] = sc, c
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------
THRESHOLD = 2.0


def make_inputs(B, S, seed):
    """Logits on a 0.25 grid (ties in the top-n, in the key and exactly at the threshold), wordpiece-like maps with multi-piece
    and repeated words, and the special rows:
      row 0               a padded position holds the maximum of both lists, the first token ([CLS]) the runner-up;
      row 1 (B >= 3)      every pair is filtered (all sums below the threshold)        -> all-zero outputs;
      row 2 (B >= 3)      two in-map tokens clear the threshold, the rest cannot       -> fewer survivors than n_best / 2."""
    rng = np.random.default_rng(seed)
    sl = (rng.integers(-8, 17, (B, S)) * 0.25).astype(np.float32)   # -2 .. 4
    el = (rng.integers(-8, 17, (B, S)) * 0.25).astype(np.float32)
    wi = np.full((B, S), -1, np.int32)
    wk = np.full((B, S), -1, np.int32)
    for b in range(B):
        length = S if S <= 3 else int(rng.integers(max(3, S // 2), S + 1))  # tokens 0 and length-1 are [CLS] / [SEP]
        vocab = max(2, (length - 2) // 3)                                    # few distinct strings: words repeat
        w = -1
        for t in range(1, length - 1):
            if w < 0 or rng.random() > 0.35:                                 # ~1/3 of the tokens continue the word before
                w += 1
                key = int(rng.integers(0, vocab))
            wi[b, t], wk[b, t] = w, key
    if S > 3:
        sl[0, S - 1] = el[0, S - 1] = 9.0
        wi[0, S - 1] = wk[0, S - 1] = -1
        sl[0, 0] = el[0, 0] = 8.5
    if B >= 3:
        sl[1], el[1] = np.minimum(sl[1], 0.75), np.minimum(el[1], 1.0)       # best sum 1.75 < 2.0
        sl[2], el[2] = np.minimum(sl[2], 0.5), np.minimum(el[2], 0.5)
        if S > 3:
            sl[2, 1] = el[2, 1] = 1.0                                        # (1,1) passes exactly at the threshold ...
            el[2, 2] = 1.25                                                  # ... and (1,2) above it
    return sl, el, wi, wk


def table():
    """(id, B, S, n_best, max_len, use_heuristics, nms, keyed): every S x B of the issue's table; n_best, max_len, the two
    switches and key / positional de-duplication rotate so that each value meets each S and each B at least once."""
    rows = []
    Ss, Bs, Ns = (9, 64, 70, 128, 512), (1, 3, 70), (1, 5, 20, 32)
    k = 0
    for S in Ss:
        for B in Bs:
            for rep in range(2):
                n_best = Ns[(k + rep * 2) % 4]
                max_len = (1, 12)[(k // 2 + rep) % 2]
                heur = (k + rep) % 2
                nms = (k // 3 + rep) % 2
                keyed = (k // 5 + rep) % 3 != 0
                rows.append((f"S{S}-B{B}-n{n_best}-L{max_len}-h{heur}-nms{nms}-{'key' if keyed else 'pos'}", B, S, n_best, max_len,
                             heur, nms, keyed))
            k += 1
    # every (n_best, max_len, heuristics, nms) combination at one multi-block shape
    for n_best in Ns:
        for max_len in (1, 12):
            for heur in (0, 1):
                for nms in (0, 1):
                    rows.append((f"S70-B3-n{n_best}-L{max_len}-h{heur}-nms{nms}-key", 3, 70, n_best, max_len, heur, nms, True))
    return rows


TABLE = table()
