"""CPU side of the word-level tagging head: the restatement of wordpool_cases.py against a brute-force walk
on every case, what the case table promises to contain, the eager pooling used by the model tests' hand composition, and the
label / tag helpers of mtvaf_amd.words and mtvaf_amd.spans (plain torch: they run on host tensors)."""
import pytest
import torch

import wordpool_cases as WC


def _index(case):
    mask, t2w, W = WC.make_index_inputs(case)
    return mask, t2w, W, WC.index_reference(mask, t2w, W)


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_restatement_matches_the_brute_force_walk(case):
    mask, t2w, W, ref = _index(case)
    brute = WC.index_brute(mask, t2w, W)
    assert set(ref) == set(brute)
    for k in ref:
        assert ref[k].dtype == brute[k].dtype and torch.equal(ref[k], brute[k]), k
    # what follows from the rule: a prefix word mask, the columns tile the live tokens in order, [CLS] is column 0
    wm = ref["word_mask"].long()
    assert torch.equal(wm, torch.cumprod(wm, dim=1))
    assert torch.equal(wm.sum(1), ref["n_cols"].long().clamp_max(W))
    for b, n in enumerate(case["lengths"]):
        k = int(wm[b].sum())
        ends = (ref["col_start"][b, :k] + ref["col_len"][b, :k]).tolist()
        assert ref["col_start"][b, :k].tolist() == ([0] + ends[:-1] if k else [])
        if int(ref["n_cols"][b]) <= W:
            assert (ends[-1] if k else 0) == n
        assert not k or (int(ref["col_len"][b, 0]) == 1 and int(ref["word_id"][b, 0]) == -1)


def test_case_table_holds_the_shapes_and_layouts_it_names():
    assert {c["S"] for c in WC.CASES} >= {1, 2, 7, 64, 65, 512} and {c["H"] for c in WC.CASES} >= {1, 20, 64, 768}
    assert all(len(c["lengths"]) <= 4 for c in WC.CASES)
    refs = [_index(c) for c in WC.CASES]
    assert any(0 in c["lengths"] for c in WC.CASES) and any(1 in c["lengths"] for c in WC.CASES)
    assert any(int(r["col_len"].max()) >= 5 for _, _, _, r in refs)
    assert any(bool((r["n_cols"] > W).any()) for _, _, W, r in refs), "a case overflows its width"
    assert any(W > m.shape[1] for m, _, W, _ in refs), "a case is wider than the sentence"
    # identity: every live token its own column
    assert any(any(int(r["n_cols"][b]) == n > 2 for b, n in enumerate(c["lengths"])) for c, (_, _, _, r) in zip(WC.CASES, refs))
    # all mapped tokens in one word: three columns over a long sentence
    assert any(any(int(r["n_cols"][b]) == 3 and n > 10 for b, n in enumerate(c["lengths"])) for c, (_, _, _, r) in zip(WC.CASES, refs))
    # truncation: the last live token is a continuation piece of a mapped word
    assert any(any(n > 1 and int(t[b, n - 1]) >= 0 and int(t[b, n - 1]) == int(t[b, n - 2]) for b, n in enumerate(c["lengths"]))
               for c, (_, t, _, _) in zip(WC.CASES, refs))
    # equal map values on both sides of a hole are two columns
    hole = [(m, t, r) for c, (m, t, _, r) in zip(WC.CASES, refs) if "hole" in c["id"]][0]
    t, r = hole[1][0].tolist(), hole[2]
    s = next(i for i in range(1, len(t) - 1) if t[i] < 0 and t[i - 1] >= 0 and t[i - 1] == t[i + 1])
    cols = r["col_of_token"][0]
    assert int(cols[s - 1]) + 2 == int(cols[s]) + 1 == int(cols[s + 1])
    # garbage behind the mask: some masked entry of some case is neither -1 nor small
    assert any(bool(((t.long().abs() > 10 ** 6) & (m == 0)).any()) for m, t, _, _ in refs)


@pytest.mark.parametrize("mode", WC.MODES)
def test_eager_pooling_agrees_with_the_restatement(mode):
    for case in WC.CASES[:6]:
        mask, t2w, W, ref = _index(case)
        x = WC.make_x(case)
        y64, _ = WC.pool_reference(x, ref, mode)
        got = WC.eager_pool(x.double(), ref, mode)
        assert torch.allclose(got, y64, rtol=1e-13, atol=1e-300), case["id"]
        # and its autograd gradient is the gather the backward kernel is held to
        dy = WC.make_x(case, seed=1, width=W)
        xg = x.double().requires_grad_(True)
        (WC.eager_pool(xg, ref, mode) * dy.double()).sum().backward()
        dx64, _ = WC.pool_bwd_reference(dy, ref, mode)
        assert torch.allclose(xg.grad, dx64, rtol=1e-13, atol=1e-300), case["id"]


def _as_index(ref):
    from mtvaf_amd.words import WordIndex
    return WordIndex(**ref)


X_ID, PAD = 8, 0


def _x_labelled(case, ref):
    """Piece-level labels as the reference's features carry them: a tag on every column's first piece, X on the continuation
    pieces, PAD behind the mask."""
    mask, t2w, W = WC.make_index_inputs(case)
    B, S = mask.shape
    gen = torch.Generator().manual_seed(3)
    labels = torch.randint(1, 8, (B, S), generator=gen)
    cols = ref["col_of_token"].long()
    start = ref["col_start"].long().gather(1, cols.clamp_min(0))
    cont = (cols >= 0) & (start != torch.arange(S)[None, :])
    labels[cont] = X_ID
    labels[cols < 0] = PAD
    return labels


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_label_helpers_round_trip(case):
    from mtvaf_amd.words import tags_to_pieces, word_allowed, word_labels
    mask, t2w, W, ref = _index(case)
    idx = _as_index(ref)
    labels = _x_labelled(case, ref)
    wl = word_labels(labels, idx)
    assert wl.shape == (mask.shape[0], W) and wl.dtype == labels.dtype
    assert not bool(wl[ref["word_mask"] == 0].any()), "0 on dead columns"
    assert not bool((wl == X_ID).any()), "no word carries X"
    back = tags_to_pieces(wl, idx, fill=X_ID, pad=PAD)
    if bool((ref["n_cols"] <= W).all()):
        assert torch.equal(back, labels)
    else:  # tokens of dropped columns come back as padding
        kept = ref["col_of_token"] >= 0
        assert torch.equal(back[kept], labels[kept]) and not bool(back[~kept].any())
    allowed = torch.randint(1, 2 ** 40, labels.shape, generator=torch.Generator().manual_seed(5))
    wa = word_allowed(allowed, idx)
    assert torch.equal(wa[ref["word_mask"] != 0], allowed.gather(1, ref["col_start"].long())[ref["word_mask"] != 0])
    assert not bool(wa[ref["word_mask"] == 0].any())


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_word_starts_from_labels_reproduces_the_maps_columns(case):
    from mtvaf_amd.spans import word_starts_from_labels
    mask, t2w, W, ref = _index(case)
    synthetic = word_starts_from_labels(_x_labelled(case, WC.index_reference(mask, t2w, mask.shape[1])), X_ID, mask)
    assert synthetic.dtype == torch.int32 and not bool((synthetic[mask == 0] != -1).any())
    again = WC.index_reference(mask, synthetic, W)
    for k in ("col_start", "col_len", "col_of_token", "word_mask", "n_cols"):
        assert torch.equal(again[k], ref[k]), k


def test_helpers_refuse_what_does_not_fit():
    from mtvaf_amd.words import WordPooling, tags_to_pieces, word_labels
    mask, t2w, W, ref = _index(WC.CASES[2])
    idx = _as_index(ref)
    with pytest.raises(ValueError):
        word_labels(torch.zeros(mask.shape[0], mask.shape[1] + 1, dtype=torch.long), idx)
    with pytest.raises(ValueError):
        tags_to_pieces(torch.zeros(mask.shape[0], W + 1, dtype=torch.long), idx, fill=X_ID)
    with pytest.raises(ValueError):
        WordPooling("max")
    assert idx.width == W
