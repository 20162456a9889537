"""CPU side of the constrained CRF entry points: the float64 reference of crf_lattice_cases pinned against enumeration of
all paths and against the unconstrained oracle, the set builders of mtvaf_amd.constraints against hand-written answers, and
the argument checks of the Python surface and the workspace query (host logic: no GPU call)."""
import pytest
import torch

import crf_lattice_cases as X
import crf_wide_cases as W
from oracle import mtvaf_oracle as O


# ---- 1. the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.BRUTE, ids=str)
@pytest.mark.parametrize("pattern", ["a", "b", "c", "e"])
def test_reference_against_enumeration(case, pattern):
    B, S, C, seed, lengths = case
    inp = W.crf_inputs(B, S, C, seed, lengths=list(lengths))
    allowed, em = X.sets((B, S, C, 1), pattern, inp)
    ref = X.make_reference((em,) + inp[1:], allowed)
    logz_a, logz, marg = X.bruteforce(em, allowed, *inp[2:])
    for name, want in (("logz_a", logz_a), ("logz", logz), ("marg", marg), ("pllh", logz_a - logz)):
        assert float((ref.r64[name] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    # the float64 Viterbi: its path is allowed and no allowed path scores higher (enumeration again)
    tags, lens, score = X.viterbi(em, allowed, *inp[2:])
    assert lens.tolist() == list(lengths)
    assert float((X.path_score(em, tags, *inp[2:]) - score).abs().max()) <= 1e-12
    emd, sd, ed, td = (x.double() for x in (em, inp[3], inp[4], inp[5]))
    for b in range(B):
        n = lengths[b]
        assert all(bool(ref.sets[b, t, tags[b, t]]) for t in range(n)) and bool((tags[b, n:] == -1).all())
        paths = torch.cartesian_prod(*[torch.arange(C)] * n).reshape(-1, n)
        sc = sd[paths[:, 0]] + emd[b, 0, paths[:, 0]] + ed[paths[:, -1]]
        ok = ref.sets[b, 0, paths[:, 0]]
        for t in range(1, n):
            sc = sc + td[paths[:, t - 1], paths[:, t]] + emd[b, t, paths[:, t]]
            ok = ok & ref.sets[b, t, paths[:, t]]
        assert abs(float(sc[ok].max()) - float(score[b])) <= 1e-12


def test_reference_tie_rule_on_a_hand_built_sentence():
    """All scores zero: every path ties, so the answer is the lowest allowed tag at every column."""
    em, start, end, trans = torch.zeros(1, 4, 5), torch.zeros(5), torch.zeros(5), torch.zeros(5, 5)
    mask = torch.tensor([[1, 1, 1, 0]], dtype=torch.uint8)
    allowed = torch.tensor([[0b10100, 0, 0b01010, 0b00001]])
    tags, lens, score = X.viterbi(em, allowed, mask, start, end, trans)
    assert tags.tolist() == [[2, 0, 1, -1]] and lens.tolist() == [3] and float(score) == 0.0


@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (3, 2, 64, 1), (3, 65, 11, 6)], ids=str)
def test_reference_with_singletons_is_the_log_likelihood(shape):
    ref = X.reference(shape, "b")
    em, tags, mask, start, end, trans = ref.inputs
    em_, s_, e_, t_ = (x.double().clone().requires_grad_(True) for x in (em, start, end, trans))
    llh = O.crf_log_likelihood(em_, tags, mask, s_, e_, t_, "none")
    grads = torch.autograd.grad((llh * ref.w.double()).sum(), [em_, s_, e_, t_])
    scale = max(1.0, float(ref.r64["logz"].abs().max()))
    assert float((ref.r64["pllh"] - llh.detach()).abs().max()) <= 1e-11 * scale
    for name, g in zip(("dem", "dstart", "dend", "dtrans"), grads):
        assert float((ref.r64[name] - g).abs().max()) <= 1e-11 * scale, name


def test_float32_reference_meets_the_rule_and_full_sets_cost_nothing():
    for pattern in X.PATTERNS:
        ref = X.reference((3, 17, 11, 1), pattern)
        for name in X.QUANTITIES:
            assert float((ref.r32[name].double() - ref.r64[name]).abs().max()) <= ref.bound[name], (pattern, name)
            assert bool(torch.isfinite(ref.r64[name]).all())
    a, e = X.reference((3, 17, 11, 1), "a"), X.reference((3, 17, 11, 1), "e")
    # (autograd sums the two chains' transition gradients in different orders: zero up to float64 rounding there)
    assert bool((a.r64["pllh"] == 0).all()) and bool((a.r64["dem"] == 0).all()) and float(a.r64["dtrans"].abs().max()) < 1e-13
    assert bool(a.sets.all()) and bool(e.sets.all()) and not torch.equal(a.allowed, e.allowed)


# ---- 2. the builders -------------------------------------------------------------------------------------------------------
def test_tag_words():
    from mtvaf_amd.constraints import full_word, tag_word
    assert tag_word([0, 3]) == 9 and tag_word([]) == 0 and tag_word([63]) == -(1 << 63)
    assert full_word(1) == 1 and full_word(11) == 2047 and full_word(64) == -1
    with pytest.raises(ValueError):
        tag_word([64])
    with pytest.raises(ValueError):
        full_word(65)


def test_sets_from_labels():
    from mtvaf_amd.constraints import sets_from_labels
    labels = torch.tensor([[0, 3, -100, 11], [10, 2, 2, -1]], dtype=torch.int32)
    got = sets_from_labels(labels, 11, unknown=(2,))
    assert got.dtype == torch.int64 and got.tolist() == [[1, 8, 0, 0], [1024, 0, 0, 0]]
    assert sets_from_labels(torch.tensor([[63, 62]]), 64).tolist() == [[-(1 << 63), 1 << 62]]
    with pytest.raises(ValueError):
        sets_from_labels(labels, 65)
    with pytest.raises(ValueError):
        sets_from_labels(labels.float(), 11)


def test_structural_sets():
    from mtvaf_amd.constraints import structural_sets
    lmap = {"O": 1, "B-PER": 2, "I-PER": 3, "X": 4, "[CLS]": 5, "[SEP]": 6}     # ids 0 .. 6; 0 is PAD
    mask = torch.tensor([[1, 1, 1, 1, 1, 0], [1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]])
    words = torch.tensor([[0, 1, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]])
    word, x, cls, sep = 0b0001110, 1 << 4, 1 << 5, 1 << 6
    got = structural_sets(lmap, mask, words)
    assert got.dtype == torch.int64
    assert got.tolist() == [[cls, word, x, word, sep, 0], [cls, word, sep, 0, 0, 0], [cls, 0, 0, 0, 0, 0]]
    assert structural_sets(lmap, mask).tolist() == [[cls, word, word, word, sep, 0], [cls, word, sep, 0, 0, 0], [cls, 0, 0, 0, 0, 0]]
    # a map without X: the piece columns stay unconstrained, and X's bit is no longer taken out of the word columns
    del lmap["X"]
    word = 0b0011110                                                             # (id 4 is a hole: it reads as PAD elsewhere)
    assert structural_sets(lmap, mask, words).tolist() == [[cls, word, 0, word, sep, 0], [cls, word, sep, 0, 0, 0],
                                                           [cls, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        structural_sets(lmap, mask, words[:, :3])


# ---- 3. argument checks ----------------------------------------------------------------------------------------------------
def test_python_surface_rejects_bad_arguments():
    from mtvaf_amd import hip
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(5, batch_first=True)
    em, ok = torch.zeros(2, 7, 5), torch.zeros(2, 7, dtype=torch.int64)
    calls = (crf.partial_llh, crf.constrained_marginals, crf.decode_constrained)
    for f in calls:
        with pytest.raises(ValueError, match="int64"):
            f(em, ok.int())
        with pytest.raises(ValueError, match="int64"):
            f(em, ok.float())
        with pytest.raises(ValueError):
            f(em, ok[:, :6])
        with pytest.raises(ValueError):
            f(em, ok[0])
        with pytest.raises(ValueError, match="S=513"):
            f(torch.zeros(1, 513, 5), torch.zeros(1, 513, dtype=torch.int64))
        with pytest.raises(ValueError):
            f(em, ok, mask=torch.ones(2, 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="reduction"):
        crf.partial_llh(em, ok, reduction="max")
    with pytest.raises(ValueError, match="C=65"):
        hip.crf_lattice_check(torch.zeros(2, 7, 65), ok)
    with pytest.raises(NotImplementedError):
        CRF(65)


def test_workspace_query_is_zero_for_rejected_shapes():
    from mtvaf_amd import hip
    q = hip.lib().mtvaf_crf_lattice_workspace_bytes
    assert q(2, 7, 5) > 0 and q(1, 1, 1) > 0 and q(3, 512, 64) >= 4 * (4 * 3 * 512 * 64)
    for B, S, C in ((2, 7, 65), (2, 513, 5), (2, 0, 5), (2, 7, 0), (0, 7, 5)):
        assert q(B, S, C) == 0, (B, S, C)
