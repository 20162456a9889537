"""Entity counting: a deliberately sequential restatement of the rule `mtvaf_entity_counts` implements, the label sets and the case
generator of the tests.  The restatement walks each sentence's kept labels in a Python loop that carries `prev` and `begin`,
straight from the predicates on label NAMES: no tables, no bit sets, nothing shared with mtvaf_amd.metrics.

A label is a pair (name, is_o).  is_o is decided by id (the map's 'O') -- the "reference" scheme asks nothing else about O, the
"seqeval" scheme reads names only.  The sentence boundary is ("O", True)."""
from __future__ import annotations

import numpy as np

SET_A = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]                  # from 1 (+ PAD): C = 11
SET_B = ["O", "EQ", "B-POS", "I-POS", "E-POS", "S-POS", "B-NEG", "I-NEG", "E-NEG", "S-NEG", "B-NEU", "I-NEU", "E-NEU", "S-NEU",
         "[CLS]", "[SEP]"]                                                                               # from 0: C = 16
SET_C = ["[CLS]", "O"] + [f"{k}-T{t:02d}" for t in range(15) for k in "BIES"] + ["X", "[SEP]"]             # from 0: C = 64 ([CLS], id 0, reads PAD)
SKIP = ("X", "[SEP]")
BOUNDARY = ("O", True)


def label_map(which):
    if which == "a":
        return {n: i for i, n in enumerate(SET_A, 1)}
    if which == "b":
        return {n: i for i, n in enumerate(SET_B, 0)}
    assert which == "c" and len(SET_C) == 64
    return {n: i for i, n in enumerate(SET_C, 0)}


def labels_of(lmap):
    """id -> (name, is_o) for ids 0 .. C-1, named as mtvaf_amd.metrics.label_sequences names them (id 0 and holes: "PAD")."""
    id2 = {i: n for n, i in lmap.items()}
    id2[0] = "PAD"
    C = max(id2) + 1
    return [(id2.get(i, "PAD"), i == lmap["O"]) for i in range(C)]


# ---- the predicates ------------------------------------------------------------------------------------------------------
def ref_class(lab):
    return lab[0].split("-")[0]


def ref_type(lab):
    return "O" if lab[1] else lab[0].split("-")[-1]


def se_tag(lab):
    return lab[0][0]


def se_type(lab):
    return lab[0][1:].split("-", 1)[-1] or "_"


def is_start(scheme, p, c):
    if scheme == "reference":
        return (not c[1]) and (p[1] or ref_type(p) != ref_type(c) or ref_class(c) == "B")
    tp, tc = se_tag(p), se_tag(c)
    if tc in ("B", "S"):
        return True
    if (tp, tc) in (("E", "E"), ("E", "I"), ("S", "E"), ("S", "I"), ("O", "E"), ("O", "I")):
        return True
    return tc not in ("O", ".") and se_type(p) != se_type(c)


def is_end(scheme, p, c):
    if scheme == "reference":
        return (not p[1]) and (c[1] or ref_type(p) != ref_type(c) or ref_class(c) == "B")
    tp, tc = se_tag(p), se_tag(c)
    if tp in ("E", "S"):
        return True
    if (tp, tc) in (("B", "B"), ("B", "S"), ("B", "O"), ("I", "B"), ("I", "S"), ("I", "O")):
        return True
    return tp not in ("O", ".") and se_type(p) != se_type(c)


def type_name(scheme, lab):
    return ref_type(lab) if scheme == "reference" else se_type(lab)


def chunks(scheme, seq):
    """seq: one sentence's kept labels -> [(type, begin, end)] with inclusive ends; begin None = unopened."""
    out, begin, prev = [], None, BOUNDARY
    for j, cur in enumerate(seq):
        if is_start(scheme, prev, cur):
            begin = j
        nxt = seq[j + 1] if j + 1 < len(seq) else BOUNDARY
        if is_end(scheme, cur, nxt):
            out.append((type_name(scheme, cur), begin, j))
        prev = cur
    return out


def name_chunks(scheme, names):
    """chunks() of a list of label names ('O' by name: the maps of these tests that go through names number from 1)."""
    return chunks(scheme, [(n, n == "O") for n in names])


def count_sequences(scheme, y_true, y_pred):
    """-> ({type: [predicted, gold, correct]}, tokens_equal, tokens_kept) over paired lists of kept-label sentences"""
    per, equal, kept = {}, 0, 0
    for gs, ps in zip(y_true, y_pred):
        assert len(gs) == len(ps)
        kept += len(gs)
        equal += sum(g == p for g, p in zip(gs, ps))
        gc, pc = chunks(scheme, gs), chunks(scheme, ps)
        for t, _, _ in pc:
            per.setdefault(t, [0, 0, 0])[0] += 1
        for t, _, _ in gc:
            per.setdefault(t, [0, 0, 0])[1] += 1
        opened = {c for c in gc if c[1] is not None}
        for c in pc:
            if c[1] is not None and c in opened:
                per[c[0]][2] += 1
    return per, equal, kept


def kept_sequences(lmap, gold, pred, mask, skip=SKIP):
    """The kept labels of every sentence, walked column by column as the trainer's loop walks them: from column 1 while the mask
    is 1, not past the first 0; a column whose gold label is skipped is dropped on both sides; an id outside [0, C) reads as 0."""
    labs = labels_of(lmap)
    C = len(labs)
    y_true, y_pred = [], []
    for b in range(gold.shape[0]):
        gs, ps = [], []
        for c in range(1, gold.shape[1]):
            if not mask[b, c]:
                break
            g, p = int(gold[b, c]), int(pred[b, c])
            if 0 <= g < C and labs[g][0] in skip:
                continue
            gs.append(labs[g if 0 <= g < C else 0])
            ps.append(labs[p if 0 <= p < C else 0])
        y_true.append(gs)
        y_pred.append(ps)
    return y_true, y_pred


def restate(lmap, scheme, gold, pred, mask, skip=SKIP):
    return count_sequences(scheme, *kept_sequences(lmap, gold, pred, mask, skip))


def counter(types, restated):
    """The restatement's result laid out as the device counter of a scorer whose type list is `types`."""
    per, equal, kept = restated
    assert set(per) <= set(types), (sorted(per), types)
    out = np.zeros(len(types) * 3 + 2, dtype=np.int64)
    for t, v in per.items():
        out[3 * types.index(t):3 * types.index(t) + 3] = v
    out[-2:] = equal, kept
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------
MASKS = ("full", "ragged", "hole", "zero_row", "col0")
PREDS = ("equal", "uniform", "mixed", "wild")


def make_mask(rng, kind, B, S):
    m = np.ones((B, S), dtype=np.uint8)
    if kind == "ragged":
        lens = rng.integers(1, S + 1, B)
        lens[0] = S  # a last kept column that is the last column
        m = (np.arange(S)[None, :] < lens[:, None]).astype(np.uint8)
    elif kind == "hole":
        for b in range(B):
            if S > 2:
                m[b, int(rng.integers(2, S))] = 0  # 1,1,..,0,1,..: nothing behind the first 0 counts
    elif kind == "zero_row":
        m[B // 2] = 0
    elif kind == "col0":
        m[:, 1:] = 0
    return m


def make_case(rng, lmap, B, S, mask_kind="ragged", pred_kind="mixed", skip_density=0.3, skip=SKIP):
    """-> gold [B,S] int64, pred [B,S] int32 (-1 behind the mask, as the Viterbi kernel pads), mask [B,S] uint8"""
    labs = labels_of(lmap)
    C = len(labs)
    skip_ids = [i for i in range(C) if labs[i][0] in skip]
    plain = [i for i in range(C) if i not in skip_ids]
    mask = make_mask(rng, mask_kind, B, S)
    gold = rng.choice(plain, size=(B, S)).astype(np.int64)
    if skip_ids and skip_density > 0:
        hit = rng.random((B, S)) < skip_density
        gold[hit] = rng.choice(skip_ids, size=int(hit.sum()))
    if pred_kind == "equal":
        pred = gold.copy()
    else:
        pred = rng.integers(0, C, (B, S)).astype(np.int64)
        if pred_kind != "uniform":
            agree = rng.random((B, S)) < 0.5  # half the columns agree: chunks that match are not rare
            pred[agree] = gold[agree]
    if pred_kind == "wild":
        w = rng.random((B, S))
        pred[w < 0.1] = -1
        pred[(w >= 0.1) & (w < 0.2)] = C + rng.integers(0, 3)
        gold[(w >= 0.2) & (w < 0.25)] = C + 5  # the rule covers both sides
        gold[(w >= 0.25) & (w < 0.3)] = -1
    pred = np.where(mask.astype(bool), pred, -1).astype(np.int32)
    return gold, pred, mask


def long_skip_case(lmap, S=256):
    """One entity with a run of >= 70 skipped columns inside it, so the previous kept column lies more than one 64-bit word back;
    an entity across columns 63 | 64; one that ends at 63 on the gold side and at 64 on the predicted side.  Needs S >= 200."""
    labs = [n for n, _ in labels_of(lmap)]
    first = [n for n in labs if n[:2] == "B-"][0]
    ty = first[2:]
    b, i, o = labs.index(first), labs.index("I-" + ty), lmap["O"]
    x = labs.index("X") if "X" in labs else labs.index("[SEP]")
    gold = np.full((3, S), o, dtype=np.int64)
    gold[0, 10], gold[0, 11:90], gold[0, 90:93] = b, x, i      # B, 79 skipped columns, I I I
    gold[0, 120], gold[0, 121:195], gold[0, 195] = b, x, b     # B, 74 skipped, B: the end of the first needs the next kept column
    gold[1, 60], gold[1, 61:67] = b, i                         # columns 60 .. 66
    gold[2, 61], gold[2, 62:64] = b, i                         # gold ends at 63
    pred = gold.astype(np.int32)
    pred[0, 90] = o                                            # the predicted entity of sentence 0 ends at column 10
    pred[2, 64] = i                                            # pred ends at 64
    return gold, pred, np.ones((3, S), dtype=np.uint8)
