"""Aspect-score fixture: drives the REAL reference `modules/eval_metrics.py::eval_absa` (imported from the reference checkout in the
authoring container through the shim of gen_golden.py) on synthetic examples / features / results and records its inputs and the
counts it returns:

    python tests/golden/gen_span_score_fixture.py        # writes tests/golden/span_score_ref.npz

Per case c (a batch of B sentences):
    c{c}_span_starts / span_ends / label_masks [B,N] int64     the predicted slots handed to the reference as RawFinalResult
    c{c}_logits [B,N,K] fp32 (integer-valued)                   their arg-max is the cls_pred handed to the reference
    c{c}_gold_starts / gold_ends / gold_class / gold_masks [B,G] int64   the feature's lists, as models/utils.py:304-335 builds them
    c{c}_word_index / c{c}_word_key [B,S] int32
    c{c}_counts = [common, retrieved, relevant]                 what eval_absa returned
Numbers only: nothing of the reference's text is stored.

The sentences are plain lower-case made-up words (no articles, no punctuation), some split into two or three pieces and many
repeated.  The reference compares normalised TEXTS; `mtvaf_span_counts` compares word-key signatures.  Predictions and gold terms
start on first pieces and end on last pieces, and the generator ASSERTS that for every (prediction, gold term) pair it uses,
signature equality is the reference's exact_match_score on wrapped_get_final_text against the term text.  A gold term the
feature truncated (its tokens lie beyond the sequence) stays in the example's term_texts -- the reference counts it in
`relevant` -- and reaches the scorer as the slot (0, 0) with mask 1, which is invalid ([CLS] is outside the word map); its words
occur nowhere else in the sentence, so that the reference cannot match its text either.
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
VOCAB = [a + b for a in SYLL[:4] for b in SYLL[4:8]] + SYLL[8:]  # 20 strings; most of the first 16 split into pieces
FAR = ["quxel", "wibon"]                                         # the words of a truncated term: used nowhere else
S, N, NG, K, B = 24, 8, 4, 4, 4
POLARITY = {1: "neutral", 2: "positive", 3: "negative"}          # models/utils.py:16 label_to_id, without 'other' / 'conflict'
#        duplicate gold texts, truncated gold term, sparse (three gold terms and one copy: common below both totals)
CASES = [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, False, True),
         (True, True, True)]


def sentence(rng, small):
    """-> words, tokens (with [CLS] / [SEP]), token_to_orig_map, first token and last token of every word"""
    n_words = int(rng.integers(5, 9))
    words = [VOCAB[int(rng.integers(0, 6 if small else len(VOCAB)))] for _ in range(n_words)]
    tokens, t2o, first, last = ["[CLS]"], {}, [], []
    for w, word in enumerate(words):
        pieces = [word[:2], "##" + word[2:]] if len(word) > 3 and rng.random() < 0.8 else [word]
        if len(word) > 4 and len(pieces) == 2 and rng.random() < 0.5:
            pieces = [word[:2], "##" + word[2:3], "##" + word[3:]]
        first.append(len(tokens))
        for p in pieces:
            t2o[len(tokens)] = w
            tokens.append(p)
        last.append(len(tokens) - 1)
    tokens.append("[SEP]")
    assert len(tokens) <= S
    return words, tokens, t2o, first, last


def main():
    G.install_shim()
    import models.utils as RU
    from modules.eval_metrics import eval_absa
    from squad.squad_evaluate import exact_match_score
    from span_propose_cases import signature
    from mtvaf_amd import spans

    log = logging.getLogger("fixture")
    rng = np.random.default_rng(20241019)
    out = {"n_cases": np.int64(len(CASES))}
    vocab = {}
    seen = dict(partial=False, dup=False, wrong_polarity=False, truncated=False)
    for c, (dup, trunc, sparse) in enumerate(CASES):
        examples, features, results = [], [], []
        ss, se, lm = (np.zeros((B, N), np.int64) for _ in range(3))
        gs, ge, gc, gm = (np.zeros((B, NG), np.int64) for _ in range(4))
        logits = rng.integers(-3, 3, (B, N, K)).astype(np.float32)
        wi = np.full((B, S), -1, np.int32)
        wk = np.full((B, S), -1, np.int32)
        for b in range(B):
            words, tokens, t2o, first, last = sentence(rng, small=(b % 2 == 1))
            W = len(words)

            def word_span():
                a = int(rng.integers(0, W))
                return a, min(W - 1, a + int(rng.integers(0, 3)))

            # gold terms in word coordinates, as the reader makes them: (first word, last word, polarity)
            terms = [(*word_span(), int(rng.integers(1, 4))) for _ in range(3 if sparse else int(rng.integers(1, 3)))]
            if dup and b == 0:                       # two gold terms of equal text: the same word twice in the sentence
                a = terms[0][0]
                words2 = list(words)
                other = (a + 2) % W
                words2[other] = words[a]
                # rebuild the sentence around the repeated word with the same piece rule
                tokens, t2o, first, last = ["[CLS]"], {}, [], []
                for w, word in enumerate(words2):
                    pieces = [word[:2], "##" + word[2:]] if len(word) > 3 else [word]
                    first.append(len(tokens))
                    for p in pieces:
                        t2o[len(tokens)] = w
                        tokens.append(p)
                    last.append(len(tokens) - 1)
                tokens.append("[SEP]")
                assert len(tokens) <= S
                words = words2
                terms = [(a, a, 2), (other, other, 2)] + terms[1:2]
            all_words = list(words)
            if trunc and b == 1:                     # a term whose words the feature does not hold: cut by the sequence length
                all_words = words + FAR
                terms = terms + [(W, W + 1, 3)]
            term_texts = [" ".join(all_words[a:z + 1]) for a, z, _ in terms]
            polarities = [POLARITY[p] for _, _, p in terms]
            # the feature's lists (models/utils.py:304-335): a truncated term has no start / end index, its label and mask stay
            kept = [(first[a], last[z]) for a, z, _ in terms if z < W]
            for g, (a, z, p) in enumerate(terms):
                gc[b, g], gm[b, g] = p, 1
            for g, (s, e) in enumerate(kept):
                gs[b, g], ge[b, g] = s, e
            assert len(terms) <= NG

            # predictions: copies of gold terms with the right or another polarity, and other word spans
            cls_pred = []
            for n in range(N):
                lm[b, n] = int(n < 6 and (n < 2 or rng.random() < 0.8))
                r = rng.random()
                if n < (1 if sparse else len(kept)):
                    a, z, p = terms[n]
                    if c % 2 == 1 and b == 2 and n == 0:
                        p = p % 3 + 1                # the matching prediction carries another polarity
                        lm[b, n] = 1
                elif r < 0.4 and not sparse:
                    a, z, p = terms[int(rng.integers(0, len(kept)))]
                    if rng.random() < 0.3:
                        p = p % 3 + 1
                else:
                    a, z = word_span()
                    p = int(rng.integers(0, 4))
                ss[b, n], se[b, n] = first[a], last[z]
                logits[b, n, p] = 4.0                # above the random integers: the arg-max
                cls_pred.append(int(np.argmax(logits[b, n])))
                assert cls_pred[-1] == p

            ids, vocab = spans.word_keys([words], vocab)
            row = spans.token_to_word(t2o, S)
            wi[b] = row.numpy()
            wk[b] = spans.token_word_keys(row[None], ids)[0].numpy()
            examples.append(types.SimpleNamespace(example_id=f"{c}-{b}", sent_tokens=all_words, term_texts=term_texts,
                                                  polarities=polarities))
            feat = types.SimpleNamespace(example_index=b, unique_id=1000 + b, tokens=tokens, token_to_orig_map=t2o)
            features.append(feat)
            results.append(RU.RawFinalResult(unique_id=1000 + b, start_indexes=ss[b].tolist(), end_indexes=se[b].tolist(),
                                             cls_pred=cls_pred + [0] * (N - len(cls_pred)), span_masks=lm[b].tolist()))

            # the premise of the comparison, on every (prediction, gold term) pair of the sentence
            for n in range(N):
                if not lm[b, n]:
                    continue
                text = RU.wrapped_get_final_text(examples[b], feat, int(ss[b, n]), int(se[b, n]), True, False, log)
                sig = signature(wi[b], wk[b], int(ss[b, n]), int(se[b, n]))
                for g, (a, z, p) in enumerate(terms):
                    em = bool(exact_match_score(text, term_texts[g]))
                    if z >= W:
                        assert not em, (text, term_texts[g])
                        continue
                    gsig = signature(wi[b], wk[b], int(gs[b, g]), int(ge[b, g]))
                    assert em == (sig == gsig), (text, term_texts[g], sig, gsig)
                    if em and RU.id_to_label[cls_pred[n]] != polarities[g]:
                        seen["wrong_polarity"] = True
            if len(set(term_texts)) < len(term_texts):
                seen["dup"] = True
            if any(z >= W for _, z, _ in terms):
                seen["truncated"] = True
                g = [z >= W for _, z, _ in terms].index(True)
                assert g == len(terms) - 1 and gm[b, g] == 1 and (gs[b, g], ge[b, g]) == (0, 0) and wi[b, 0] < 0

        metrics, _ = eval_absa(examples, features, results, True, False, log)
        common, retrieved, relevant = (int(metrics[k]) for k in ("common", "retrieved", "relevant"))
        assert 0 < common, c
        assert retrieved == int(lm.sum()) and relevant == int(gm.sum())
        seen["partial"] |= common < retrieved and common < relevant
        for name, v in (("span_starts", ss), ("span_ends", se), ("label_masks", lm), ("logits", logits), ("gold_starts", gs),
                        ("gold_ends", ge), ("gold_class", gc), ("gold_masks", gm), ("word_index", wi), ("word_key", wk)):
            out[f"c{c}_{name}"] = v
        out[f"c{c}_counts"] = np.array([common, retrieved, relevant], np.int64)
        print(f"case {c}: dup {dup} trunc {trunc} sparse {sparse}: common {common} retrieved {retrieved} relevant {relevant}")
    assert all(seen.values()), seen   # the cases are not degenerate
    path = os.path.join(HERE, "span_score_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
