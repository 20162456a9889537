"""Calibration counting (csrc/calibration.hip, include/mtvaf_hip.h: mtvaf_chunk_calibration / mtvaf_entity_calibration): a plain
Python / NumPy restatement of the contract and the case builder of the tests.

The restatement chunks the gold labels with one loop over the two tables (carrying the last start), bins a log-probability by
counting the fp32 edges it reaches with ``>=``, and accumulates everything in Python ints and float64: no bit sets, no ordinals
shared with the kernel.

The kernel-level cases use a label set small enough to read: ids 0..6 = PAD, O, B-A, I-A, B-B, I-B, X (C = 7) and three types
"_" (everything that is no entity label), "A", "B".  Seven ids leave no room for [CLS] / [SEP] of their own: column 0 carries PAD
and the last column of a sentence X, which is what those columns are to a chunker -- labels that are not entities.  The tables
are STRICT BIO: only B- starts a chunk, so an I- behind O ends a chunk that was never opened, the case the kernel must drop."""
from __future__ import annotations

import numpy as np

NAMES = ["PAD", "O", "B-A", "I-A", "B-B", "I-B", "X"]
TYPES = ["_", "A", "B"]
C, T = len(NAMES), len(TYPES)
PAD, O, BA, IA, BB, IB, X = range(7)


def _ent(l):
    return l < C and "-" in NAMES[l]


def strict_bio_tables():
    """-> start, end uint8 [(C+1),(C+1)] indexed [prev][cur] (index C = the sentence boundary, an O), type_of int32 [C+1]"""
    n = C + 1
    start, end = np.zeros((n, n), np.uint8), np.zeros((n, n), np.uint8)
    for p in range(n):
        for c in range(n):
            start[p, c] = _ent(c) and NAMES[c][0] == "B"
            end[p, c] = _ent(p) and not (_ent(c) and NAMES[c][0] == "I" and NAMES[c][2:] == NAMES[p][2:])
    type_of = np.array([TYPES.index(NAMES[l][2:]) if _ent(l) else 0 for l in range(n)], np.int32)
    return start, end, type_of


def edges_for(n_bins):
    """fp32 [n_bins + 1]: -inf, log(k / n_bins), 0 -- written out here, not taken from the package"""
    e = [-np.inf] + [np.log(k / n_bins) for k in range(1, n_bins)] + [0.0]
    return np.array(e, dtype=np.float32)


def bin_of(lp, edges):
    nb = len(edges) - 1
    return int(sum(1 for k in range(1, nb) if np.float32(lp) >= edges[k]))


def kept_columns(mask_row, keep_row):
    L = 0
    while L < len(mask_row) and mask_row[L]:
        L += 1
    return [c for c in range(L) if (keep_row[c] != 0 if keep_row is not None else c >= 1)]


def gold_chunks(gold_row, cols, start, end, type_of, n_labels):
    """-> [(type, start ordinal, end ordinal)] over the kept columns ``cols``: every end with a start at or before it"""
    labs = [int(gold_row[c]) if 0 <= int(gold_row[c]) < n_labels else 0 for c in cols]
    out, begin = [], None
    for j, l in enumerate(labs):
        prev = labs[j - 1] if j > 0 else n_labels
        nxt = labs[j + 1] if j + 1 < len(labs) else n_labels
        if start[prev][l]:
            begin = j
        if end[l][nxt] and begin is not None:
            out.append((int(type_of[l]), begin, j))
    return out


class Counts:
    """The counter block as named arrays"""

    def __init__(self, n_types, n_bins):
        self.n = np.zeros((n_types, n_bins), np.int64)
        self.hit = np.zeros((n_types, n_bins), np.int64)
        self.gold = np.zeros(n_types, np.int64)
        self.reach = np.zeros(n_types, np.int64)
        self.sum_p = np.zeros((n_types, n_bins), np.float64)
        self.sum_sq = np.zeros((n_types, n_bins), np.float64)
        self.sentences = 0

    def ints(self):
        return np.concatenate([self.n.ravel(), self.hit.ravel(), self.gold, self.reach, [self.sentences]])

    def add_item(self, t, lp, hit, edges, dead=False):
        k = 0 if dead else bin_of(lp, edges)
        p = 0.0 if dead else float(np.exp(np.float64(lp)))
        self.n[t, k] += 1
        self.hit[t, k] += int(hit)
        self.sum_p[t, k] += p
        self.sum_sq[t, k] += (p - float(hit)) ** 2


def _gold_side(out, gold, mask, keep, tables, width):
    start, end, type_of = tables
    n_labels = len(type_of) - 1
    per_sentence = []
    for s in range(gold.shape[0]):
        cols = kept_columns(mask[s], None if keep is None else keep[s])
        chunks = gold_chunks(gold[s], cols, start, end, type_of, n_labels)
        for t, b, e in chunks:
            out.gold[t] += 1
            if width is None or e - b + 1 <= width:
                out.reach[t] += 1
        per_sentence.append((cols, set(chunks)))
    out.sentences += gold.shape[0]
    return per_sentence


def reference_events(log_post, gold, mask, keep, tables, edges, out=None):
    """mtvaf_chunk_calibration restated; ``out``: a Counts to add into"""
    B, S, W, n_types = log_post.shape
    out = out or Counts(n_types, len(edges) - 1)
    for s, (cols, chunks) in enumerate(_gold_side(out, gold, mask, keep, tables, W)):
        for b in range(S):
            for w in range(W):
                for t in range(n_types):
                    lp = log_post[s, b, w, t]
                    if not lp > -np.inf:  # -inf and NaN
                        continue
                    hit = b in cols and (t, cols.index(b), cols.index(b) + w) in chunks
                    out.add_item(t, lp, hit, edges)
    return out


def reference_entities(ents, log_conf, gold, mask, keep, tables, edges, n_types, out=None):
    """mtvaf_entity_calibration restated"""
    S = gold.shape[1]
    out = out or Counts(n_types, len(edges) - 1)
    for s, (cols, chunks) in enumerate(_gold_side(out, gold, mask, keep, tables, None)):
        for slot, (b, e, t) in enumerate(ents[s]):
            if not (0 <= b < S and 0 <= e < S and 0 <= t < n_types):
                continue
            hit = b in cols and e in cols and (int(t), cols.index(b), cols.index(e)) in chunks
            lc = log_conf[s, slot]
            out.add_item(int(t), lc, hit, edges, dead=not lc > -np.inf)
    return out


# ---- the kernel-level cases: B = 3, S = 12, C = 7, W = 4, T = 3, NB = 8, E = 6 ------------------------------------------------
B, S, W, NB, E = 3, 12, 4, 8, 6


def gold_case():
    """gold [3,12] int64, mask / keep [3,12] uint8.
    sentence 0 (mask all ones): A over columns 1..6 with column 3 NOT kept -- 5 kept columns wide, wider than W = 4; B at 8..9;
                                an A of one column at 10; X in the last column.
    sentence 1 (length 1):      no kept column at all.
    sentence 2 (length 9):      I-B at 1..2 behind the boundary (an end without a start: dropped), A at 4..5 with a non-kept
                                column 5 inside (the chunk ends at the kept column 6), label ids outside [0, C) at 7."""
    gold = np.full((B, S), O, np.int64)
    mask = np.zeros((B, S), np.uint8)
    keep = np.zeros((B, S), np.uint8)
    gold[0, 0], gold[0, 1], gold[0, 2:7], gold[0, 8], gold[0, 9], gold[0, 10], gold[0, 11] = PAD, BA, IA, BB, IB, BA, X
    mask[0, :] = 1
    keep[0, 1:11] = 1
    keep[0, 3] = 0
    mask[1, 0] = 1
    mask[2, :9] = 1
    gold[2, 0], gold[2, 1:3], gold[2, 4], gold[2, 5:7], gold[2, 7], gold[2, 8] = PAD, IB, BA, IA, 99, X
    keep[2, 1:8] = 1
    keep[2, 5] = 0
    keep[2, 10] = 1  # behind the sentence: does not count
    return gold, mask, keep


def events_case(seed=0):
    """-> log_post [3,12,4,3] fp32 (random log-probabilities, NOT a chain's), gold, mask, keep, edges.  Planted: the gold events
    that fit W, an element exactly on an edge, a NaN, -inf elements, finite values at non-kept and masked start columns."""
    rng = np.random.default_rng(seed)
    edges = edges_for(NB)
    gold, mask, keep = gold_case()
    lp = np.log(rng.uniform(1e-4, 1.0, (B, S, W, T))).astype(np.float32)
    lp[rng.random((B, S, W, T)) < 0.3] = -np.inf
    lp[0, 8, 1, 2] = np.float32(np.log(0.9))   # B at 8..9: a hit in the top bin
    lp[0, 10, 0, 1] = edges[4]                 # A at 10: a hit EXACTLY on an edge -- bin 4, not 3
    lp[0, 1, 3, 1] = np.float32(np.log(0.7))   # the widest event from column 1 ends at column 5: the gold chunk ends at 6, a miss
    lp[2, 4, 1, 1] = np.float32(np.log(0.6))   # A at 4..6 over the non-kept 5: width 2 in kept columns, a hit
    lp[2, 1, 1, 2] = np.float32(np.log(0.5))   # the unopened I-B I-B: no gold chunk, a miss
    lp[0, 2, 0, 0] = np.nan
    lp[1, 0, 0, 0] = np.float32(np.log(0.3))   # the sentence without kept columns still has scored items
    lp[0, 3, 0, 1] = np.float32(np.log(0.2))   # a non-kept start column
    return lp, gold, mask, keep, edges


def entities_case():
    """-> ents [3,6,3] int32, log_conf [3,6] fp32, gold, mask, keep, edges: hits, misses, unused slots, a -inf confidence, a type
    out of range, columns out of range, a duplicate (both count, both hit)."""
    edges = edges_for(NB)
    gold, mask, keep = gold_case()
    ents = np.full((B, E, 3), -1, np.int32)
    conf = np.zeros((B, E), np.float32)
    ents[0, 0], conf[0, 0] = (1, 6, 1), np.log(0.95)      # the wide A: a hit here (no width limit)
    ents[0, 1], conf[0, 1] = (8, 9, 2), np.log(0.8)       # B: a hit
    ents[0, 2], conf[0, 2] = (8, 9, 2), np.log(0.4)       # the same span again: counts again, hits again
    ents[0, 3], conf[0, 3] = (8, 9, 1), np.log(0.3)       # the wrong type: a miss
    ents[0, 4], conf[0, 4] = (10, 10, 1), -np.inf         # a hit without a confidence: bin 0, p = 0
    ents[0, 5], conf[0, 5] = (10, 10, 3), np.log(0.9)     # type out of range: skipped
    ents[1, 0], conf[1, 0] = (0, 0, 1), np.log(0.5)       # a prediction in the sentence without kept columns: a miss
    ents[1, 1], conf[1, 1] = (3, 12, 1), np.log(0.5)      # end column out of range: skipped
    ents[2, 0], conf[2, 0] = (4, 6, 1), edges[2]          # a hit exactly on an edge
    ents[2, 1], conf[2, 1] = (1, 2, 2), np.log(0.7)       # the unopened I-B I-B: dropped on the gold side, a miss
    ents[2, 2], conf[2, 2] = (4, 5, 1), np.nan            # ends at the non-kept column: a miss; NaN -> bin 0, p = 0
    return ents, conf, gold, mask, keep, edges


def valid_bio(rng, lmap, n_rows, n_cols):
    """Gold labels in which every end has a start, over a map with O, B-t / I-t, X, [CLS], [SEP]: -> gold int64, mask uint8"""
    types = sorted({n[2:] for n in lmap if n[:2] == "B-"})
    gold = np.zeros((n_rows, n_cols), np.int64)
    mask = np.zeros((n_rows, n_cols), np.uint8)
    for r in range(n_rows):
        L = n_cols if r == 0 else int(rng.integers(3, n_cols + 1))
        mask[r, :L] = 1
        gold[r, 0], gold[r, L - 1] = lmap["[CLS]"], lmap["[SEP]"]
        inside = None
        for c in range(1, L - 1):
            u = rng.random()
            if inside is not None and u < 0.2:
                gold[r, c] = lmap["X"]  # a continuation piece: skipped, the entity goes on
            elif inside is not None and u < 0.6:
                gold[r, c] = lmap["I-" + inside]
            elif u < 0.8:
                inside = types[int(rng.integers(len(types)))]
                gold[r, c] = lmap["B-" + inside]
            else:
                inside, gold[r, c] = None, lmap["O"]
    return gold, mask
