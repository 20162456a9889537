"""Candidate-span fixture: drives the REAL reference `models/utils.py::span_annotate_candidates` (eval branch, imported from the
reference checkout in the authoring container through the shim of gen_golden.py) on synthetic examples / features and records
its inputs and the lists it returns:

    python tests/golden/gen_span_candidates_fixture.py        # writes tests/golden/span_candidates_ref.npz

Per case c (a batch of B sentences and one set of the trainer's switches):
    c{c}_start_logits / c{c}_end_logits [B,S] fp32 (multiples of 0.25)   c{c}_word_index / c{c}_word_key [B,S] int32
    c{c}_scalars = [n_best_size, max_answer_length, use_heuristics, use_nms, filter_type == 'em']   c{c}_threshold fp32
    c{c}_span_starts / span_ends / labels / label_masks [B,n_best_size] int64  -- what the reference returned
Numbers only: nothing of the reference's text is stored.

The sentences are plain lower-case made-up words (no articles, no punctuation), some split into two or three pieces and many
repeated.  The reference compares candidate TEXTS; `mtvaf_span_propose` compares word-key signatures.  A span that starts or
ends inside a word has a partial text in the reference (get_final_text projects the pieces) but whole-word keys, so here inner
pieces carry a start / end logit no pair can pass the threshold with, as a trained extraction head gives them; the generator
ASSERTS that on every pair that can pass, signature equality is the reference's text equality and a shared key is its f1 > 0.
"""
from __future__ import annotations

import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import gen_golden as G  # noqa: E402

SYLL = ["ba", "ko", "mi", "ru", "zet", "lop", "dax", "fim", "gur", "hul", "vok", "nep"]
S = 24
LOW = -50.0  # inner pieces: no pair with this logit passes any threshold used here
#        n_best, max_len, heuristics, use_nms, filter_type, threshold
CASES = [(20, 12, True, False, "f1", 2.0),
         (20, 12, True, True, "f1", 2.0),
         (20, 12, False, True, "em", 2.0),
         (5, 3, True, False, "f1", 1.0),
         (7, 1, False, False, "f1", 3.0),
         (32, 12, True, True, "f1", 0.5),
         (1, 12, True, False, "f1", 2.0),
         (32, 4, False, False, "em", 2.5)]
B = 4


def sentence(rng, full):
    """-> words, tokens (with [CLS] / [SEP]), token_to_orig_map, first-piece and last-piece flags per token"""
    n_words = int(rng.integers(4, 9))
    vocab = [a + b for a in SYLL[:4] for b in SYLL[4:8]] + SYLL[8:]           # 20 strings; 16 of them split into two pieces
    words = [vocab[int(rng.integers(0, len(vocab) if not full else 6))] for _ in range(n_words)]
    tokens, t2o, first, last = ["[CLS]"], {}, [False], [False]
    for w, word in enumerate(words):
        pieces = [word[:2], "##" + word[2:]] if len(word) > 3 and rng.random() < 0.8 else [word]
        if len(word) > 4 and len(pieces) == 2 and rng.random() < 0.5:
            pieces = [word[:2], "##" + word[2:3], "##" + word[3:]]
        for k, p in enumerate(pieces):
            t2o[len(tokens)] = w
            tokens.append(p)
            first.append(k == 0)
            last.append(k == len(pieces) - 1)
    tokens.append("[SEP]")
    first.append(False)
    last.append(False)
    assert len(tokens) <= S
    return words, tokens, t2o, first, last


def main():
    G.install_shim()
    import models.utils as RU
    from squad.squad_evaluate import f1_score
    from span_propose_cases import signature
    from mtvaf_amd import spans

    log = logging.getLogger("fixture")
    rng = np.random.default_rng(20240611)
    out = {"n_cases": np.int64(len(CASES))}
    vocab = {}
    for c, (n_best, max_len, heur, use_nms, ftype, thr) in enumerate(CASES):
        examples, features, results = [], [], []
        sl = (rng.integers(-8, 17, (B, S)) * 0.25).astype(np.float32)
        el = (rng.integers(-8, 17, (B, S)) * 0.25).astype(np.float32)
        wi = np.full((B, S), -1, np.int32)
        wk = np.full((B, S), -1, np.int32)
        for b in range(B):
            words, tokens, t2o, first, last = sentence(rng, full=(b == 1))
            for t in range(len(tokens)):
                if t in t2o and not first[t]:
                    sl[b, t] = LOW
                if t in t2o and not last[t]:
                    el[b, t] = LOW
            if b == 2:      # a padded position holds the row maximum of both lists, [CLS] the runner-up
                sl[b, S - 1] = el[b, S - 1] = 9.0
                sl[b, 0] = el[b, 0] = 8.5
            if b == 3:      # few survivors: only the first word's pieces can pass
                keep = [t for t in t2o if t2o[t] == 0]
                for t in range(S):
                    if t not in keep:
                        sl[b, t], el[b, t] = min(sl[b, t], -4.0), min(el[b, t], -4.0)
                sl[b, keep[0]], el[b, keep[-1]] = 3.0, 3.0
            ids, vocab = spans.word_keys([words], vocab)
            row = spans.token_to_word(t2o, S)
            wi[b] = row.numpy()
            wk[b] = spans.token_word_keys(row[None], ids)[0].numpy()
            examples.append(types.SimpleNamespace(sent_tokens=words))
            feat = types.SimpleNamespace(example_index=b, unique_id=1000 + b, tokens=tokens, token_to_orig_map=t2o)
            features.append(feat)
            results.append(RU.RawSpanResult(unique_id=1000 + b, start_logits=sl[b].tolist(), end_logits=el[b].tolist()))

            # the premise of the comparison, on every pair that can pass the threshold
            assert float(max(sl[b].max(), el[b].max())) + LOW < thr
            cand = [(s, e) for s in t2o for e in t2o if first[s] and last[e] and e >= s]
            texts = {p: RU.wrapped_get_final_text(examples[b], feat, p[0], p[1], True, False, log) for p in cand}
            sigs = {p: signature(wi[b], wk[b], p[0], p[1]) for p in cand}
            for p in cand:
                for r in cand:
                    assert (texts[p] == texts[r]) == (sigs[p] == sigs[r]), (texts[p], texts[r])
                    assert (f1_score(texts[p], texts[r]) > 0) == bool(set(sigs[p]) & set(sigs[r])), (texts[p], texts[r])

        st, en, lab, lm = RU.span_annotate_candidates(examples, features, results, ftype, "eval", heur, use_nms, thr, n_best,
                                                      max_len, True, False, log)
        out[f"c{c}_start_logits"], out[f"c{c}_end_logits"] = sl, el
        out[f"c{c}_word_index"], out[f"c{c}_word_key"] = wi, wk
        out[f"c{c}_scalars"] = np.array([n_best, max_len, int(heur), int(use_nms), int(ftype == "em")], np.int64)
        out[f"c{c}_threshold"] = np.float32(thr)
        for name, v in (("span_starts", st), ("span_ends", en), ("labels", lab), ("label_masks", lm)):
            out[f"c{c}_{name}"] = np.array(v, np.int64)
        print(f"case {c}: n_best {n_best} max_len {max_len} heur {heur} nms {use_nms}/{ftype} thr {thr}: accepted per sentence",
              np.array(lm).sum(1).tolist())
    path = os.path.join(HERE, "span_candidates_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
