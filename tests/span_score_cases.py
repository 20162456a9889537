"""Aspect scoring of the span model: a plain Python restatement of the rule `mtvaf_span_counts` implements, and the case table the
GPU tests run it over.  The restatement follows the written rule (include/mtvaf_hip.h), not the kernel:
per-sentence lists, tuples as signatures, one loop per bullet.

    score(...)   a batch -> dict(counts [3K+2] int64, pred_class [B,N] int32, matched_gold [B,N] int32)
    counter layout: per class retrieved, relevant, common; then relevant_other, sentences
"""
from __future__ import annotations

import numpy as np

from span_propose_cases import signature


def valid(word_index, s, e):
    S = len(word_index)
    return 0 <= s <= e < S and word_index[s] >= 0 and word_index[e] >= 0


def score(span_starts, span_ends, label_masks, logits, gold_starts, gold_ends, gold_class, gold_masks, word_index, word_key=None):
    """span_* / label_masks [B,N], logits [B,N,K], gold_* [B,G], word_index [B,S], word_key [B,S] or None (= word_index)."""
    B, N, K = logits.shape
    G = gold_starts.shape[1]
    counts = [0] * (3 * K + 2)
    pred_class = np.full((B, N), -1, np.int32)
    matched_gold = np.full((B, N), -1, np.int32)
    for b in range(B):
        wi = [int(x) for x in word_index[b]]
        wk = wi if word_key is None else [int(x) for x in word_key[b]]
        golds = []  # (slot, signature, class) of the gold slots that can be matched
        for g in range(G):
            if gold_masks[b, g] == 0:
                continue
            c, s, e = int(gold_class[b, g]), int(gold_starts[b, g]), int(gold_ends[b, g])
            if 0 <= c < K:
                counts[3 * c + 1] += 1
            else:
                counts[3 * K] += 1
            if valid(wi, s, e):
                golds.append((g, signature(wi, wk, s, e), c))
        for n in range(N):
            if label_masks[b, n] == 0:
                continue
            row = [float(x) for x in logits[b, n]]
            c = min(k for k in range(K) if not any(other > row[k] for other in row))
            pred_class[b, n] = c
            counts[3 * c] += 1
            s, e = int(span_starts[b, n]), int(span_ends[b, n])
            if not valid(wi, s, e):
                continue
            sig = signature(wi, wk, s, e)
            hits = [g for g, gsig, gc in golds if gsig == sig and gc == c]
            if hits:
                counts[3 * c + 2] += 1
                matched_gold[b, n] = min(hits)
        counts[3 * K + 1] += 1
    return dict(counts=np.array(counts, np.int64), pred_class=pred_class, matched_gold=matched_gold)


def totals(counts, K):
    """-> (common, retrieved, relevant) as eval_absa sums them: over every class, relevant with the out-of-range gold classes."""
    c = [int(x) for x in counts]
    return sum(c[2:3 * K:3]), sum(c[0:3 * K:3]), sum(c[1:3 * K:3]) + c[3 * K]


# ---- the case table ---------------------------------------------------------------------------------------------------------
def make_inputs(B, S, N, G, K, seed):
    """Wordpiece-like maps with multi-piece and repeated words (few distinct keys: equal signatures at different positions are
    common), logits on a 0.5 grid (ties), and per sentence a mix of slots: copies of gold spans (same or another class, shifted
    onto an inner piece of the same word), random spans, spans that end outside the map or the sentence, padding slots.  Gold
    classes run over -1 .. K (both ends outside the range).  Special rows:
      row 0               every slot of both sides exists (N * G pairs), the first gold span covers S - 2 tokens;
      row 1 (B >= 3)      no predicted slot exists;
      row 2 (B >= 3)      no gold slot exists."""
    rng = np.random.default_rng(seed)
    wi = np.full((B, S), -1, np.int32)
    wk = np.full((B, S), -1, np.int32)
    ss, se, lm = (np.zeros((B, N), np.int64) for _ in range(3))
    gs, ge, gc, gm = (np.zeros((B, G), np.int64) for _ in range(4))
    logits = (rng.integers(-4, 5, (B, N, K)) * 0.5).astype(np.float32)
    for b in range(B):
        length = S if S <= 3 or b == 0 else int(rng.integers(max(3, S // 2), S + 1))  # tokens 0 and length-1: [CLS] / [SEP]
        lo, hi = (1, length - 2) if length >= 3 else (0, length - 1)                  # S < 3: every token is in the map
        vocab = max(2, (hi - lo + 1) // 4)
        w, key = -1, 0
        for t in range(lo, hi + 1):
            if w < 0 or rng.random() > 0.35:
                w += 1
                key = int(rng.integers(0, vocab))
            wi[b, t], wk[b, t] = w, key

        def rand_span():
            s = int(rng.integers(lo, hi + 1))
            return s, min(hi, s + int(rng.integers(0, 4)))

        for g in range(G):
            gm[b, g] = int(b == 0 or rng.random() < 0.7)
            gs[b, g], ge[b, g] = rand_span()
            gc[b, g] = int(rng.integers(-1, K + 1)) if rng.random() < 0.25 else int(rng.integers(0, K))
            kind = rng.random()
            if kind < 0.1:
                gs[b, g], ge[b, g] = 0, 0                                # a truncated term: the padding values with mask 1
            elif kind < 0.15:
                ge[b, g] = S + int(rng.integers(0, 3))                   # an end beyond the sentence
            elif kind < 0.2:
                gs[b, g], ge[b, g] = ge[b, g], gs[b, g] - 1              # e < s
        if b == 0:
            gs[b, 0], ge[b, 0], gc[b, 0] = lo, hi, 1                     # S - 2 tokens wide (S >= 3)
        for n in range(N):
            lm[b, n] = int(b == 0 or rng.random() < 0.75)
            kind = rng.random()
            if kind < 0.5:                                               # a gold span, usually with the gold class on top
                g = int(rng.integers(0, G))
                s, e = int(gs[b, g]), int(ge[b, g])
                if 0 <= s <= e < S and rng.random() < 0.5:               # start on another piece of the same word
                    while s + 1 <= e and wi[b, s + 1] == wi[b, s] and wi[b, s] >= 0 and rng.random() < 0.7:
                        s += 1
                ss[b, n], se[b, n] = s, e
                if 0 <= gc[b, g] < K and rng.random() < 0.7:
                    logits[b, n, int(gc[b, g])] = 2.0 if rng.random() < 0.5 else 2.5   # 2.0 ties with the grid's top value
            elif kind < 0.85:
                ss[b, n], se[b, n] = rand_span()
            elif kind < 0.9:
                ss[b, n], se[b, n] = -1, int(rng.integers(0, S))
            elif kind < 0.95:
                ss[b, n], se[b, n] = hi, S + 1
            else:
                ss[b, n], se[b, n] = 0, 0                                # propose_spans' padding values with mask 1: [CLS]
    if B >= 3:
        lm[1] = 0
        gm[2] = 0
    return dict(span_starts=ss, span_ends=se, label_masks=lm, logits=logits, gold_starts=gs, gold_ends=ge, gold_class=gc,
                gold_masks=gm, word_index=wi, word_key=wk)


def table():
    """(id, B, S, N, G, K, keyed): every S and every B of the issue's table crossed; N, G, K and keyed / positional signatures
    rotate so that each value meets each S and each B at least once; then the full shape (32 x 32 pairs, S = 512)."""
    rows = []
    Ss, Bs, Ns, Gs, Ks = (3, 24, 64, 65, 130, 512), (1, 3, 70), (1, 5, 20, 32), (1, 4, 32), (2, 4, 5, 8)
    k = 0
    for S in Ss:
        for B in Bs:
            N, G, K, keyed = Ns[k % 4], Gs[(k + k // 3) % 3], Ks[(k + k // 4) % 4], k % 2 == 0
            rows.append((f"S{S}-B{B}-N{N}-G{G}-K{K}-{'key' if keyed else 'pos'}", B, S, N, G, K, keyed))
            k += 1
    for N, G, K, keyed in ((32, 32, 8, True), (32, 32, 2, False), (1, 1, 4, True), (20, 4, 4, True), (5, 32, 5, False)):
        rows.append((f"S512-B3-N{N}-G{G}-K{K}-{'key' if keyed else 'pos'}", 3, 512, N, G, K, keyed))
    return rows


TABLE = table()
