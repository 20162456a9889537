"""presplit_cases.py deserves to be the reference of test_presplit_contract_gpu.py: its split is exact wherever the planes stay in
bf16's normal range, loses no more than the documented floor below it, its two image layouts are permutations of the same planes,
and the edge classes sit where their names say (no GPU)."""
import pytest
import torch

import presplit_cases as PC

KS = [64, 96]


def _sum64(x):
    return torch.stack([p.double() for p in PC.split3(x)]).sum(0)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", PC.X3_CASES)
def test_every_plane_is_finite(case, K):
    for x in PC.operands(case, 128, 128, K, seed=K):
        assert all(bool(torch.isfinite(p.float()).all()) for p in PC.split3(x)), case


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", PC.X3_CASES)
def test_the_planes_sum_to_the_element_exactly_in_the_normal_range(case, K):
    """h + m + l == x exactly (float64) for every element of at least 2^-109, in all eight cases; below it the split loses at most
    2^-133.  Whole operands lie above the limit except the tiny operand of the two subnormal-plane cases -- and B of near_fp32_max
    (randn 2^-110), which test_gemm_f32_split_adversarial holds to the plain bound all the same: its loss, at most 2^-134 per element
    against |a| < 2^128, stays far inside 2^-24 (4 + sqrt K) |A|.|B|."""
    A, B = PC.operands(case, 128, 128, K, seed=K)
    below = {"tiny_times_one": (True, False), "huge_times_tiny": (False, True), "near_fp32_max": (False, True)}.get(case, (False, False))
    for x, has_below in zip((A, B), below):
        normal = x.abs() >= PC.NORMAL_MIN
        s = _sum64(x)
        assert torch.equal(s[normal], x.double()[normal]), case
        assert float((s - x.double()).abs().max()) <= PC.PLANE_FLOOR
        assert bool((~normal).any()) == has_below, case
    if case == "near_fp32_max":
        err = (_sum64(A) @ _sum64(B) - A.double() @ B.double()).abs()
        assert bool((err <= PC.error_bound(case, A, B, K)).all())  # (no floor added for this case)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", PC.SUBNORMAL_PLANE_CASES)
def test_subnormal_planes_keep_the_documented_floor(case, K):
    """Operands below 2^-109: the product of the restated planes' sums (float64) stands where test_gemm_f32_split_adversarial has
    the kernel's result, and stays within that test's bound -- the floor K 2^-133 max|other| on top of 2^-24 (4 + sqrt K) |A|.|B|.
    Element by element the split loses at most 2^-133 there (half of it, in fact: one RNE to bf16's subnormal grid)."""
    A, B = PC.operands(case, 128, 128, K, seed=K)
    tiny = A if case == "tiny_times_one" else B
    assert float(tiny.abs().max()) < PC.NORMAL_MIN
    assert float((_sum64(tiny) - tiny.double()).abs().max()) <= PC.PLANE_FLOOR
    err = (_sum64(A) @ _sum64(B) - A.double() @ B.double()).abs()
    assert bool((err <= PC.error_bound(case, A, B, K)).all())
    assert float(err.max()) > 0  # (the split did lose something here: the floor is not vacuous)


@pytest.mark.parametrize("blocked", [False, True])
def test_image_round_trips_in_both_layouts(blocked):
    A, _ = PC.operands("elementwise_spread", 128, 128, 96, seed=1)
    img = PC.image(A, blocked)
    assert img.dtype == torch.int16 and img.shape == (3 * 128 * 96,)
    planes = PC.unlayout(img, 128, 96, blocked).view(torch.bfloat16)
    for got, want in zip(planes, PC.split3(A)):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(PC.planes_sum(img, 128, 96, blocked), A.double())
    # the two layouts hold the same words at other places: element (r, c) of plane p
    nat, blk = PC.image(A, False).view(3, 128, 96), PC.image(A, True).view(3, 3, 128, 32)
    for p, r, c in [(0, 0, 0), (1, 5, 31), (2, 127, 32), (1, 64, 95)]:
        assert nat[p, r, c] == blk[c // 32, p, r, c % 32]
    assert torch.equal(PC.layout(PC.unlayout(img, 128, 96, blocked), blocked), img)


def test_specials_hold_every_value_and_their_boundary_plane_is_finite():
    A, B = PC.operands("specials", 128, 128, 64, seed=2)
    bits = A.view(torch.int32)
    for val in PC.SPECIAL_VALUES:
        want = torch.tensor([val]).view(torch.int32)
        assert int((bits == want).sum()) >= 8, val
    assert bool((A[PC.ZERO_ROW] == 0).all()) and bool((A[:, PC.ZERO_K] == 0).all())
    assert int((bits[PC.ZERO_ROW] < 0).sum()) == 32  # (every other zero is -0)
    h, m, l = PC.split3(A)
    assert all(bool(torch.isfinite(p.float()).all()) for p in (h, m, l))
    edge = A.abs() == PC.SPLIT_MAX
    assert bool((h.float().abs()[edge] == 2.0 ** 127 * (2 - 2.0 ** -7)).all())  # bf16's largest finite number
    assert float((_sum64(A) - A.double()).abs().max()) <= PC.PLANE_FLOOR
    assert bool(torch.isfinite((A.double().abs() @ B.double().abs()).float()).all())  # (the products stay inside fp32's range)


def test_overflow_edge_first_plane_is_infinite():
    assert torch.tensor(PC.BF16_OVERFLOW).bfloat16().isinf() and torch.tensor(PC.SPLIT_MAX).bfloat16().isfinite()
    assert PC.BF16_OVERFLOW == 2.0 ** 127 * (2 - 2.0 ** -8) and PC.SPLIT_MAX < PC.BF16_OVERFLOW < PC.FLT_MAX
    M, N, K = 128, 128, 64
    A, _ = PC.operands("overflow_edge", M, N, K, seed=3)
    h, m, l = PC.split3(A)
    hit = torch.zeros(M, K, dtype=torch.bool)
    for i, j, val in PC.poison_positions("overflow_edge", M, N, K):
        assert abs(val) >= PC.BF16_OVERFLOW and A[i, j] == val
        hit[i, j] = True
    assert bool(torch.isfinite(A).all())
    assert bool(h.float().isinf()[hit].all()) and bool(l.float().isnan()[hit].all())
    assert bool(torch.isfinite(h.float())[~hit].all())


@pytest.mark.parametrize("case", ["nonfinite", "nonfinite_b"])
def test_nonfinite_elements_sit_where_the_table_says(case):
    M, N, K = 128, 256, 64
    A, B = PC.operands(case, M, N, K, seed=4)
    x = A if case == "nonfinite" else B
    pos = PC.poison_positions(case, M, N, K)
    assert int((~torch.isfinite(x)).sum()) == len(pos) == 3
    assert all(not torch.isfinite(x[i, j]) for i, j, _ in pos)
    assert len({i for i, _, _ in pos}) == 3 and len({j for _, j, _ in pos}) == 3
    assert bool(torch.isfinite(B if case == "nonfinite" else A).all())


def test_shapes_are_whole_tiles():
    assert all(M % 128 == 0 and N % 128 == 0 and K % 32 == 0 for M, N, K in PC.SHAPES)
    assert [N % 256 == 0 for _, N, _ in PC.SHAPES] == [False, True, False, True]
    assert [N % 192 == 0 for _, N, _ in PC.SHAPES] == [False, False, True, False]
