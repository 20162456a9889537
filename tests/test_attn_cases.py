"""CPU checks of what the prefix-attention contract tests stand on (attn_cases.py): the dropout-mask replica, the float64
reference against a hand-written softmax backward, and that every case has the property it was built for."""
import numpy as np
import pytest
import torch

import attn_cases as AC
from attn_cases import BY_NAME, CASES, KT


# ---------------------------------------------------------------------------------------------------------
# keep_mask
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_keep_mask_keep_fraction(p):
    keep = AC.keep_mask(5, 6, 3, 2, 70, 106, p)
    assert keep.shape == (3, 2, 70, 106) and keep.dtype == np.bool_
    assert abs(float(keep.mean()) - (1 - p)) < 0.02, float(keep.mean())
    # ... and per key tile, per sentence: no slice of the index space is left out of the hash
    for b in range(3):
        for t0 in (0, 64):
            assert abs(float(keep[b, :, :, t0:t0 + 64].mean()) - (1 - p)) < 0.03


def test_keep_mask_is_deterministic_and_depends_on_seed_offset_and_row():
    a = AC.keep_mask(5, 6, 2, 2, 33, 70, 0.3)
    assert np.array_equal(a, AC.keep_mask(5, 6, 2, 2, 33, 70, 0.3))
    for other in (AC.keep_mask(6, 6, 2, 2, 33, 70, 0.3), AC.keep_mask(5, 7, 2, 2, 33, 70, 0.3),
                  AC.keep_mask(5 + (1 << 32), 6, 2, 2, 33, 70, 0.3)):
        assert 0.3 < float((a != other).mean()) < 0.55  # two independent p = 0.3 masks differ in 2 * 0.3 * 0.7 = 0.42 of the places
    flat = a.reshape(-1, 70)
    assert all(not np.array_equal(flat[i], flat[i + 1]) for i in range(flat.shape[0] - 1))
    # the row id is (b*NH + h)*S + q: a [B, NH, S] grid is the flat row axis cut up, whatever B and NH are
    assert np.array_equal(a.reshape(-1, 70), AC.keep_mask(5, 6, 4, 1, 33, 70, 0.3).reshape(-1, 70))
    # ... and a different S shifts the rows of every (b, h) but the first
    c = AC.keep_mask(5, 6, 2, 2, 34, 70, 0.3)
    assert np.array_equal(c[0, 0, :33], a[0, 0]) and not np.array_equal(c[0, 1, :33], a[0, 1])
    assert np.array_equal(c[0, 0, 33], a[0, 1, 0])


def test_keep_mask_threshold_and_key_words():
    assert AC.drop_thr(0.0) == 0 and bool(AC.keep_mask(1, 2, 1, 1, 4, 8, 0.0).all())
    assert AC.drop_thr(0.1) == int(np.float32(0.1) * 2.0 ** 32) == 429496736  # p is a float in the ABI
    assert AC.drop_thr(0.9999999999) == 4294967040
    assert 0 <= AC.drop_key(5, 6) < 2 ** 32 and AC.drop_key(5, 6) != AC.drop_key(5, 7)
    assert AC.drop_key(5, 6) == AC.drop_key(5, 6 + (1 << 32))  # only the low word of the offset enters the key


# ---------------------------------------------------------------------------------------------------------
# reference against the closed-form backward
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("name", ["t106_two_holes", "masked_first_tile"])
def test_reference_agrees_with_closed_form_softmax_backward(name, p):
    case = BY_NAME[name]
    keep = AC.keep_mask(11, 3, case.B, case.NH, case.S, case.T, p) if p else None
    ref = AC.reference(case, keep=keep, p=p)
    hand = AC.closed_form(case, keep=keep, p=p)
    for k in ("ctx", "lse", "probs", "dqkv", "dpk", "dpv", "delta"):
        assert ref[k].dtype == torch.float64 and ref[k].shape == hand[k].shape, k
        err = float((ref[k] - hand[k]).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref[k].abs().max())), (k, err)
    assert abs(float(ref["probs"].sum(-1).min()) - 1) < 1e-12 and abs(float(ref["probs"].sum(-1).max()) - 1) < 1e-12
    dead = (ref["probs"] * (1 - AC.mask_of(case))[:, None, None, :].double()).abs().max()
    assert float(dead) == 0.0  # exp(-10000 - max) is exactly 0 in float64
    if p:
        plain = AC.reference(case)
        assert torch.equal(plain["lse"], ref["lse"]) and not torch.equal(plain["ctx"], ref["ctx"])


@pytest.mark.parametrize("c", CASES, ids=str)
def test_bf16_gradient_bounds_are_four_times_the_priced_error(c):
    """The bf16 gradient bounds are priced, not tuned: 4 x the error against float64 of the formula in fp32 torch on bf16-valued
    inputs with P rounded to bf16 before P V.  A widened bound (BF16_GRAD) is that product to two figures; everywhere else the
    product is inside the defaults."""
    norm, elem = AC.priced_bf16_grad(c)
    print(f"[attn-cases] priced bf16 gradient error {c.name}: norm-relative {norm:.3e}, element-wise {elem:.3e}")
    if c.name in AC.BF16_GRAD:
        nb, eb = AC.BF16_GRAD[c.name]
        assert 0.95 < nb / (4 * norm) < 1.05 and 0.95 < eb / (4 * elem) < 1.05, (norm, elem)
    else:
        assert 4 * norm <= 1.2e-2 and 4 * elem <= 2e-2, (norm, elem)


def test_closed_form_rounds_only_p_in_its_bf16_mode():
    """The pricing arithmetic is the issue's: bf16 P and nothing else.  With a one-key sentence P is exactly 1, rounding it is
    the identity, and the fp32 evaluation of that sentence is as close to float64 as plain fp32."""
    c = BY_NAME["s16_p0"]
    ref = AC.reference(c, bf16=True)
    a = AC.closed_form(c, bf16=True, dtype=torch.float32)
    b = AC.closed_form(c, bf16=False, dtype=torch.float32)
    x16, x32 = AC.inputs(c, bf16=True), AC.inputs(c)
    assert not torch.equal(x16["qkv"], x32["qkv"]) and torch.equal(x16["qkv"], x16["qkv"].bfloat16().float())
    row = slice(c.S, 2 * c.S)  # sentence 1: length 1
    assert AC.need(a["dqkv"][row], ref["dqkv"][row]) < 1e-5 and AC.need(a["ctx"][row], ref["ctx"][row]) < 1e-5
    assert a["ctx"].dtype == torch.float32 and not torch.equal(a["ctx"], a["ctx"].bfloat16().float())  # O is not rounded
    assert b["ctx"].shape == a["ctx"].shape


def test_reference_gradients_against_finite_differences():
    """One directional derivative of the float64 graph, so that the closed form and autograd are not wrong together."""
    case = BY_NAME["s16_p0"]
    x = AC.inputs(case)
    ref = AC.reference(case)
    g = torch.Generator().manual_seed(3)
    dirq = torch.randn(x["qkv"].shape, generator=g, dtype=torch.float64)
    q = x["qkv"].double()

    def f(eps):
        y = dict(x)
        y["qkv"] = q + eps * dirq
        qq, kk, vv = AC._heads(case, y)
        s = qq @ kk.transpose(-1, -2) * AC.SCALE + x["addmask"].double()[:, None, None, :]
        ctx = (torch.softmax(s, -1) @ vv).permute(0, 2, 1, 3).reshape(case.B * case.S, case.H)
        return float((ctx * x["dctx"].double()).sum())
    num = (f(1e-5) - f(-1e-5)) / 2e-5
    ana = float((ref["dqkv"] * dirq).sum())
    assert abs(num - ana) < 1e-7 * max(1.0, abs(ana)), (num, ana)


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def test_cases_are_small_and_named_once():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert c.NH <= 4 and c.S <= 130 and len(c.lengths) == c.B and max(c.lengths) <= c.S
        x = AC.inputs(c)
        assert x["qkv"].shape == (c.B * c.S, 3 * c.H) and x["pk"].shape == (c.B, c.NH * c.P * 64) and x["addmask"].shape == (c.B, c.T)
        assert float(x["dctx"].abs().min()) > 0.0  # dense upstream gradient, masked queries included
        for b in range(c.B):  # exempt <=> no live key at all, which takes P = 0 (both directions: a live sentence is compared)
            assert (b in c.exempt) == (not bool(x["mask"][b].any()))
            assert b not in c.exempt or c.P == 0
    assert any((c.NH * c.B) % 8 == 0 for c in CASES) and any((c.NH * c.B) % 8 for c in CASES)
    assert sum(c.suffix_masked for c in CASES) >= 5
    for c in CASES:  # the ordered launch list of a packed case is no identity
        assert not c.suffix_masked or list(c.lengths) != sorted(c.lengths, reverse=True)


def test_cases_land_where_they_say():
    c = BY_NAME["s16_p0"]
    assert (c.S, c.P) == (16, 0) and AC.effective_T(c) == [16, 1, 9]
    c = BY_NAME["t106_two_holes"]
    assert c.T == 106 and (c.T - KT + 15) // 16 == 3 and set(c.lengths) == {70, 1, 37}
    m = AC.mask_of(c)
    assert m[0, c.P + 3] == 0 and m[0, c.P + 2] == 1 and m[0, c.P + 4] == 1 and m[2, c.P] == 0 and m[2, c.P + 1] == 1
    assert AC.effective_T(c) == [106, 37, 73]
    c = BY_NAME["t128_on_tile"]
    assert c.T == 2 * KT and AC.effective_T(c) == [127, 128, 65]
    c = BY_NAME["odd_prefix_p63"]
    assert c.P % 2 == 1 and c.P % 4 == 3 and c.T == 128 and c.S - KT == 1 and AC.effective_T(c) == [64, 128]
    c = BY_NAME["three_qtiles_p1"]
    assert c.P == 1 and (c.S + KT - 1) // KT == 3 and c.S - 2 * KT == 2
    c = BY_NAME["block_edges"]
    assert c.lengths == (15, 16, 17, 48, 49) and AC.effective_T(c) == [31, 32, 33, 64, 65]
    c = BY_NAME["masked_first_tile"]
    m = AC.mask_of(c)
    assert c.P == 100 and float(m[0, :KT].sum()) == 0 and float(m[0, KT:c.P].sum()) == c.P - KT  # the first key tile, wholly
    assert 0 < float((1 - m[1, :c.P]).sum()) < 8
    c = BY_NAME["text_all_masked"]
    m = AC.mask_of(c)
    assert c.P > 0 and float(m[1, c.P:].sum()) == 0 and float(m[1, :c.P].sum()) > 0 and AC.effective_T(c)[1] == c.T
    assert AC.last_unmasked(c) == [19, -1]
    c = BY_NAME["all_masked_p0"]
    assert c.P == 0 and c.exempt == (1,) and all(not k.exempt for k in CASES if k is not c) and float(AC.mask_of(c)[1].sum()) == 0 and AC.effective_T(c)[1] == c.T


def test_masked_first_tile_running_maximum_starts_near_minus_14427():
    c = BY_NAME["masked_first_tile"]
    x = AC.inputs(c)
    q, k, _ = AC._heads(c, x)
    s2 = (q.double() @ k.double().transpose(-1, -2) * AC.SCALE + x["addmask"].double()[:, None, None, :]) * 1.4426950408889634
    first = s2[0, :, :, :KT].amax(-1)
    assert float(first.max()) < -14400 and float(first.min()) > -14450
    assert float((s2[0, :, :, KT:2 * KT].amax(-1) - first).min()) > 14000  # ... and jumps in the second tile


def _tile_maxima(c):
    x = AC.inputs(c)
    q, k, _ = AC._heads(c, x)
    s = q.double() @ k.double().transpose(-1, -2) * AC.SCALE + x["addmask"].double()[:, None, None, :]
    return torch.stack([s[..., t0:t0 + KT].amax(-1) for t0 in range(0, c.T, KT)], -1)  # [B, NH, S, tiles]


def test_steep_cases_move_the_row_maximum_across_key_tiles():
    c = BY_NAME["steep_scaled"]
    tm = _tile_maxima(c)[1]  # the full-length sentence: three key tiles
    assert tm.shape[-1] == 3 and float(tm.amax(-1).mean()) > 15  # scores of many e-folds: the softmax is nearly one-hot
    run = torch.cummax(tm, -1).values
    assert float((run[..., -1] > run[..., 0]).double().mean()) > 0.4  # the running maximum climbs behind the first tile
    c = BY_NAME["steep_ramp"]
    tm = _tile_maxima(c)
    assert tm.shape[-1] == 3
    rising = (tm[0, ..., 1] > tm[0, ..., 0]) & (tm[0, ..., 2] > tm[0, ..., 1])
    falling = (tm[1, ..., 1] < tm[1, ..., 0]) & (tm[1, ..., 2] < tm[1, ..., 1])
    assert float(rising.double().mean()) > 0.5 and float(falling.double().mean()) > 0.5, (rising.double().mean(), falling.double().mean())
    assert float((tm[0, ..., 2] - tm[0, ..., 0]).median()) > 8 and float((tm[1, ..., 0] - tm[1, ..., 2]).median()) > 8


def test_packing_helpers():
    c = BY_NAME["block_edges"]
    assert AC.cu_plain(c).tolist() == [0, 15, 31, 48, 96, 145] and AC.cu_plain(c).dtype == torch.int32
    o = AC.cu_ordered(c)
    assert o.tolist() == [-1, 15, 31, 48, 96, 145, 4, 3, 2, 1, 0] and o.dtype == torch.int32
    c = BY_NAME["s16_p0"]
    assert AC.cu_ordered(c).tolist() == [-1, 16, 17, 26, 0, 2, 1]
    rows = AC.kept_rows(c)
    assert rows.tolist() == list(range(16)) + [16] + list(range(32, 41))
    with pytest.raises(AssertionError):
        AC.cu_plain(BY_NAME["t106_two_holes"])
