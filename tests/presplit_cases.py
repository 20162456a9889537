"""The pre-split fp32 GEMM path (csrc/gemm_f32p.hip, gemm_f32pw.hip) on the host: an independent restatement of the three-way bf16
split and of both plane-image layouts, the adversarial operand classes of x3_cases.py plus three classes at the edge of the split's
domain, and the smallest shapes at which the kernels of the family still take different code paths.  test_presplit_cases.py proves
the restatement on the host; test_presplit_contract_gpu.py holds every kernel of the family to it."""
import torch

import x3_cases

X3_CASES = list(x3_cases.CASES)
SUBNORMAL_PLANE_CASES = ("tiny_times_one", "huge_times_tiny")  # (operands below 2^-109: the documented absolute floor applies)
EDGE_CASES = ["specials", "overflow_edge", "nonfinite", "nonfinite_b"]

# (M, N, K): M, N % 128 == 0, K % 32 == 0
SHAPES = [(128, 128, 32),   # one tile, one k-tile: prologue equals drain
          (128, 256, 64),   # the 128 x 256 tile, two k-tiles
          (256, 384, 96),   # the 128 x 192 tile (N % 192 == 0, N % 256 != 0); three k-tiles fill the three-stage ring
          (640, 256, 160)]  # five tile rows: a ragged last band of the tile walk; five k-tiles

NORMAL_MIN = 2.0 ** -109       # |x| >= this: all three planes are normal bf16 numbers or zero
PLANE_FLOOR = 2.0 ** -133      # bf16's smallest subnormal: what a split may lose of an element below NORMAL_MIN


def _bits(u):
    return torch.tensor([u], dtype=torch.int32).view(torch.float32)[0].item()


# RNE_bf16(x) is infinite from the midpoint between bf16's largest finite number 2^127 (2 - 2^-7) and 2^128 on (the tie goes to the
# even neighbour, 2^128): 2^127 (2 - 2^-8) = 0x7F7F8000.  Its fp32 predecessor is the largest magnitude the split can take.
BF16_OVERFLOW = _bits(0x7F7F8000)
SPLIT_MAX = _bits(0x7F7F7FFF)
FLT_MAX = _bits(0x7F7FFFFF)
SUB_MIN, SUB_MAX, NORM_MIN = _bits(0x00000001), _bits(0x007FFFFF), _bits(0x00800000)
SPECIAL_VALUES = [0.0, -0.0, SUB_MIN, SUB_MAX, NORM_MIN, SPLIT_MAX, -SPLIT_MAX]
# specials: row ZERO_ROW and reduction index ZERO_K of A hold nothing but +0 / -0
ZERO_ROW, ZERO_K = 3, 5
B_SCALE = 2.0 ** -12  # B of the edge classes: |a| <= FLT_MAX against K <= 160 such elements stays inside fp32's range


def split3(x):
    """fp32 -> the three bf16 planes (h, m, l) of the split, by torch's CPU conversions (RNE): the reference for every plane bit."""
    assert x.dtype == torch.float32 and not x.is_cuda
    h = x.bfloat16()
    r = x - h.float()
    m = r.bfloat16()
    l = (r - m.float()).bfloat16()
    return h, m, l


def layout(t3, blocked):
    """[3][rows][cols] (any dtype) -> flat, in the order of the natural image [3][rows][cols] or of the tile-blocked image
    [cols / 32][3][rows][32]."""
    _, rows, cols = t3.shape
    assert cols % 32 == 0
    if blocked:
        t3 = t3.reshape(3, rows, cols // 32, 32).permute(2, 0, 1, 3)
    return t3.contiguous().reshape(-1)


def unlayout(flat, rows, cols, blocked):
    """inverse of layout: flat image -> [3][rows][cols]"""
    if blocked:
        return flat.reshape(cols // 32, 3, rows, 32).permute(1, 2, 0, 3).reshape(3, rows, cols).contiguous()
    return flat.reshape(3, rows, cols)


def image(x, blocked):
    """The plane image of x [rows][cols] as int16 words, flat: comparable with hip.Planes(x, blocked).img.view(torch.int16)."""
    return layout(torch.stack(split3(x)).view(torch.int16), blocked)


def planes_sum(img16, rows, cols, blocked):
    """float64 sum of the three planes of an int16 image -> [rows][cols]"""
    return unlayout(img16, rows, cols, blocked).view(torch.bfloat16).double().sum(0)


def per_exponent(shape, lo, hi, g):
    """2^e with an integer exponent e in [lo, hi] drawn per element"""
    return torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).float())


def poison_positions(case, M, N, K):
    """(i, j, value) of the planted elements of `overflow_edge` / `nonfinite` (A[i][j], i a row and j a reduction index) and of
    `nonfinite_b` (B[i][j], i a reduction index and j a column)."""
    inf, nan = float("inf"), float("nan")
    if case == "overflow_edge":
        return [(1, 0, BF16_OVERFLOW), (M // 2 + 2, K // 2 + 1, -BF16_OVERFLOW), (M // 2 + 2, K - 1, _bits(0x7F7F8001)),
                (M - 2, K - 1, FLT_MAX), (M - 2, 7, -FLT_MAX)]
    if case == "nonfinite":
        return [(2, 1, inf), (M // 2 + 1, K - 1, -inf), (M - 1, K // 2, nan)]
    if case == "nonfinite_b":
        return [(1, 2, inf), (K - 1, N // 2 + 1, -inf), (K // 2, N - 1, nan)]
    raise ValueError(case)


def operands(case, M, N, K, seed):
    """-> (A [M,K], B [K,N]) fp32 CPU tensors: the eight cases of x3_cases.operands and
    specials: A sprinkled with +0, -0, the smallest and the largest fp32 subnormal, 2^-126 and +-2^127 (2 - 2^-8)(1 - 2^-24), the
      largest magnitude whose first plane stays finite; row ZERO_ROW and reduction index ZERO_K of A are all +0 / -0.
    overflow_edge: a few elements of A at and above 2^127 (2 - 2^-8), up to FLT_MAX (poison_positions).
    nonfinite / nonfinite_b: one +inf, one -inf and one NaN at known positions of A / of B (poison_positions).
    B of these classes is randn 2^-12: the fp32 product stays finite wherever its operands are."""
    if case in X3_CASES:
        return x3_cases.operands(case, M, N, K, seed)
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * B_SCALE
    if case == "specials":
        n = len(SPECIAL_VALUES)
        idx = torch.randperm(M * K, generator=g)[:n * max(8, M * K // 64)]
        flat = A.view(-1)
        for j, val in enumerate(SPECIAL_VALUES):
            flat[idx[j::n]] = val
        zeros = torch.tensor([0.0, -0.0])
        A[ZERO_ROW] = zeros[torch.arange(K) % 2]
        A[:, ZERO_K] = zeros[torch.arange(M) % 2]
    elif case in ("overflow_edge", "nonfinite"):
        for i, j, val in poison_positions(case, M, N, K):
            A[i, j] = val
    elif case == "nonfinite_b":
        for i, j, val in poison_positions(case, M, N, K):
            B[i, j] = val
    else:
        raise ValueError(case)
    return A.float().contiguous(), B.float().contiguous()


def error_bound(case, A, B, K):
    """The element-wise bound of test_gemm_f32_split_adversarial on |C - A.B|: 2^-24 (4 + sqrt K) |A|.|B|, plus the documented
    floor K 2^-133 max|other operand| where an operand has elements below 2^-109 (their second / third planes are subnormal)."""
    bound = 2.0 ** -24 * (4 + K ** 0.5) * (A.double().abs() @ B.double().abs())
    if case == "tiny_times_one" or case == "specials":
        bound = bound + K * PLANE_FLOOR * float(B.abs().max())
    elif case == "huge_times_tiny":
        bound = bound + K * PLANE_FLOOR * float(A.abs().max())
    return bound
