"""The pre-split fp32 GEMM path (csrc/gemm_f32p.hip, gemm_f32pw.hip and every kernel that writes a plane image) held to
presplit_cases.py: the split pass against the host's restatement bit for bit, every producer against the split pass on values
spread over the exponent range, every kernel of the family on the adversarial operands of x3_cases.py under the bounds of
test_gemm_f32_split_adversarial, the edge of the split's domain and non-finite operands, and mtvaf_gemm_f32p_slabs."""
import functools

import pytest
import torch

import presplit_cases as PC
import stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"

# mtvaf_f32p_wide (include/mtvaf_hip.h): a mask of the products that may leave the 128 x 128 tile -- 1 forward (128 x 256, or 128 x 192
# when N % 192 == 0), 2 dX, 4 weight gradients; 8 = never the 128 x 128 tile where another can serve.  0: the 128 x 128 tile only.
NARROW, FWD, DX, DW, NEVER_NARROW = 0, 1, 2, 4, 8
# launch-profiler keys of the family: 400 + 4 (k-major A) + 8 (k-major B) + 16 (grouped) + 32 (wide tile) + 64 (128 x 192)
KEY, KEY_A_KM, KEY_B_KM, KEY_GROUP, KEY_WIDE, KEY_192 = 400, 4, 8, 16, 32, 64


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


@pytest.fixture
def tiles(hip):
    """-> launch(mask, key, fn, splits=1): fn() under mtvaf_f32p_wide(mask); its first recorded launch must carry `key`.  The mask
    of the process is restored behind the test."""
    was = hip.f32p_wide()

    def launch(mask, key, fn, splits=1):
        hip.f32p_wide(mask)
        hip.prof_start(8)
        try:
            out = fn()
        finally:
            recs = hip.prof_stop(8)
        assert recs and (recs[0][0]["cfg"], recs[0][0]["splits"]) == (key, splits), (mask, key, splits, recs)
        return out
    try:
        yield launch
    finally:
        hip.f32p_wide(was)


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))  # (NaN-proof: an unwritten tile fails)


def words(pl):
    return pl.img.view(torch.int16)


def empty_image(hip, M, N):
    im = hip.Planes(torch.empty(M, N, device=DEV), True, fill=False)
    im.img.fill_(float("nan"))
    return im


@functools.lru_cache(maxsize=None)
def problem(case, shape, seed=11):
    """-> A, B, float64 product, |A|.|B|, element-wise bound (computed once per case and shape)"""
    M, N, K = shape
    A, B = PC.operands(case, M, N, K, seed)
    return A, B, A.double() @ B.double(), A.double().abs() @ B.double().abs(), PC.error_bound(case, A, B, K)


def pipe_product(hip, A, B):
    """A . B on the fp32 MFMA pipe (mtvaf_f32_split off)"""
    (M, K), N = A.shape, B.shape[1]
    out = nan(M, N)
    was = hip.f32_split()
    try:
        hip.f32_split(False)
        hip.gemm(A.to(DEV), 0, B.t().contiguous().to(DEV), 0, out, M, N, K)
    finally:
        hip.f32_split(was)
    return out.double().cpu()


def check(out, ref, mag, bound, e_pipe, case, label):
    """The assertions of test_gemm_f32_split_adversarial: finite, element-wise within 2^-24 (4 + sqrt K) |A|.|B| of the float64
    product (+ the floor K 2^-133 max|other| where an operand has elements below 2^-109), and -- without the floor -- not worse than
    the fp32 pipe on the same operands by that test's 1.5 x / 1.25 x margins.  e_pipe: the pipe's error / |A|.|B|."""
    assert bool(torch.isfinite(out).all()), (label, "the first plane must not round to infinity / NaN")
    err = (out.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), (label, float((err / bound).max()))
    if case in PC.SUBNORMAL_PLANE_CASES or case == "specials":
        return
    e = err / mag
    assert float(e.max()) <= 1.5 * float(e_pipe.max()) + 2.0 ** -25, (label, float(e.max()), float(e_pipe.max()))
    assert float(e.pow(2).mean().sqrt()) <= 1.25 * float(e_pipe.pow(2).mean().sqrt()) + 2.0 ** -26, label


# ---------------------------------------------------------------------------------------------------------------------
# a. the split pass against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", [False, True], ids=["natural", "blocked"])
@pytest.mark.parametrize("case", PC.X3_CASES + ["specials"])
def test_split_pass_is_the_restated_split_bit_for_bit(hip, case, blocked):
    """mtvaf_f32_split_planes against presplit_cases.split3 (torch's RNE conversions on the host), both operands of every
    adversarial case and `specials`, both layouts: every word of every plane.  Elements of at least 2^-109 (all planes normal or
    zero) first, then the rest -- elements below 2^-109, whose residuals and second / third planes are subnormal, the fp32
    subnormals and +-0 of `specials`: measured on the MI355X, the device keeps fp32 subnormal residuals and rounds to bf16's
    subnormal grid exactly as the host does, so equality is asserted there too."""
    A, B = PC.operands(case, 128, 128, 64, seed=21)
    for name, x in (("A", A), ("B", B)):
        rows, cols = x.shape
        got = words(hip.Planes(x.to(DEV), blocked)).cpu()
        want = PC.image(x, blocked)
        normal = PC.layout((x.abs() >= PC.NORMAL_MIN).expand(3, rows, cols), blocked)
        assert torch.equal(got[normal], want[normal]), (case, name, "normal range", int((got != want)[normal].sum()))
        rest = ~normal
        if bool(rest.any()):
            lost = (PC.planes_sum(got, rows, cols, blocked) - x.double()).abs()[x.abs() < PC.NORMAL_MIN]
            print(f"[split pass] {case} {name} {'blocked' if blocked else 'natural'}: {int(rest.sum()) // 3} elements below 2^-109, "
                  f"{int((got != want)[rest].sum())} plane words differ from the host, max |x - (h + m + l)| = {float(lost.max()):.3e} "
                  f"(2^-133 = {PC.PLANE_FLOOR:.3e})")
            assert float(lost.max()) <= PC.PLANE_FLOOR
            assert torch.equal(got[rest], want[rest]), (case, name, "below 2^-109", int((got != want)[rest].sum()))


# ---------------------------------------------------------------------------------------------------------------------
# b. every producer of a plane image equals the split pass on hard values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["none", "gelu"])
@pytest.mark.parametrize("case", ["elementwise_spread", "huge_times_huge", "tiny_times_tiny"])
def test_gemm_epilogue_planes_equal_the_split_pass_over_the_exponent_range(hip, tiles, case, epi):
    """mtvaf_gemm_f32p_ep with results between 2^-100 and 2^116: the image the epilogue writes is the split pass over the fp32
    result it also wrote, on the 128 x 128 and on the 128 x 256 tile, with and without the fp32 copy."""
    M, N, K = shape = PC.SHAPES[1]
    A, B, ref, _, _ = problem(case, shape)
    pa, pb = hip.Planes(A.to(DEV), True), hip.Planes(B.t().contiguous().to(DEV), True)
    bias = (rnd(N, seed=5) * float(ref.abs().mean())).float().to(DEV) if epi == "gelu" else None
    code = hip.EPI_GELU if epi == "gelu" else hip.EPI_NONE
    results = []
    for mask, key in ((NARROW, KEY), (FWD | NEVER_NARROW, KEY + KEY_WIDE)):
        for with_c in (True, False):
            got, out, pre = empty_image(hip, M, N), nan(M, N) if with_c else None, nan(M, N) if epi == "gelu" else None
            tiles(mask, key, lambda: hip.gemm_planes_ep(pa, pb, got, out=out, bias=bias, epi=code, aux=pre))
            if with_c:
                assert bool(torch.isfinite(out).all())
                want = words(hip.Planes(out, True))
                results.append(out)
            assert torch.equal(words(got), want), (case, epi, mask, with_c, int((words(got) != want).sum()))
    assert same_bits(results[0], results[1])
    top = float(results[0].abs().max())
    assert {"elementwise_spread": 1.0 < top < 2.0 ** 60, "huge_times_huge": top > 2.0 ** 100, "tiny_times_tiny": top < 2.0 ** -90}[case], top


def test_layernorm_planes_equal_the_split_pass_with_spread_gamma_and_beta(hip):
    """mtvaf_dropout_res_ln_fwd_planes / _bwd_rows_planes (test_layernorm_kernels_write_the_plane_images_of_their_outputs) with gamma
    and beta carrying per-column exponents in 2^[-60, 60]: outputs and input gradients over 120 binades, planes still those of the
    split pass over the fp32 result."""
    L_ = hip.lib()
    M, H, ns = 384, 256, 2
    g = torch.Generator().manual_seed(60)
    x, res = rnd(M, H, seed=61).to(DEV), rnd(M, H, seed=62).to(DEV)
    gamma = (rnd(H, seed=63) * PC.per_exponent((H,), -60, 60, g)).to(DEV)
    beta = (rnd(H, seed=64) * PC.per_exponent((H,), -60, 60, g)).to(DEV)
    bias = rnd(H, seed=65).to(DEV)
    slabs = rnd(ns, M, H, seed=66).to(DEV)
    E = lambda *s_: torch.empty(*s_, device=DEV)
    for nslab in (0, ns):
        o0, mu0, rs0, xo0 = E(M, H), E(M), E(M), E(M, H)
        img = empty_image(hip, M, H)
        hip._ck(L_.mtvaf_dropout_res_ln_fwd_planes(hip._p(slabs if nslab else x), nslab, hip._p(bias), hip._p(xo0), hip._p(res), hip._p(gamma),
                                                   hip._p(beta), hip._p(o0), hip._p(mu0), hip._p(rs0), M, H, 1e-12, 0.1, 77, 5, hip._p(img.img),
                                                   hip._st()), "ln planes")
        assert bool(torch.isfinite(o0).all()) and float(o0.abs().max()) > 2.0 ** 50 and float(o0.abs()[o0 != 0].min()) < 2.0 ** -50
        assert torch.equal(words(img), words(hip.Planes(o0, True))), nslab
        dout = rnd(M, H, seed=67).to(DEV)
        xin = xo0 if nslab else x
        nb = int(L_.mtvaf_ln_bwd_workspace_bytes(M, H))
        p0, p1 = torch.zeros(nb // 4, device=DEV), torch.zeros(nb // 4, device=DEV)
        dx0, dr0, dr1 = E(M, H), E(M, H), E(M, H)
        if nslab:
            hip._ck(L_.mtvaf_dropout_res_ln_bwd_rows_slabs(hip._p(dout), hip._p(slabs), nslab, hip._p(xin), hip._p(res), hip._p(gamma), hip._p(mu0),
                                                           hip._p(rs0), hip._p(dx0), hip._p(dr0), 0, M, H, 0.1, 77, 5, hip._p(p0), None, hip._st()), "b")
        else:
            hip._ck(L_.mtvaf_dropout_res_ln_bwd_rows(hip._p(dout), hip._p(xin), hip._p(res), hip._p(gamma), hip._p(mu0), hip._p(rs0), hip._p(dx0),
                                                     hip._p(dr0), 0, M, H, 0.1, 77, 5, hip._p(p0), None, hip._st()), "b")
        dimg = empty_image(hip, M, H)
        hip._ck(L_.mtvaf_dropout_res_ln_bwd_rows_planes(hip._p(dout), hip._p(slabs) if nslab else None, nslab, hip._p(xin), hip._p(res),
                                                        hip._p(gamma), hip._p(mu0), hip._p(rs0), None, hip._p(dr1), 0, M, H, 0.1, 77, 5, hip._p(p1),
                                                        hip._p(dimg.img), hip._st()), "b planes")
        assert bool(torch.isfinite(dx0).all()) and same_bits(dr0, dr1) and same_bits(p0, p1)
        assert torch.equal(words(dimg), words(hip.Planes(dx0, True))), nslab


def test_adamw_planes_shadow_is_the_split_of_the_updated_parameters_over_the_exponent_range(hip):
    """mtvaf_adamw_planes, one step, parameters with per-element exponents in 2^[-40, 40] and the magnitudes of `specials` (+-0, fp32
    subnormals, 2^-126, the largest magnitude the split takes) planted in every matrix: each shadow image is the split pass over
    the updated fp32 parameters."""
    g = torch.Generator().manual_seed(9)
    n = sum(r * c for r, c in SC.PLANES_SHAPES) + sum(SC.PLANES_GAPS)
    p = torch.randn(n, generator=g) * PC.per_exponent((n,), -40, 40, g)
    nv = len(PC.SPECIAL_VALUES)
    idx = torch.randperm(n, generator=g)[:n // 8]
    for j, val in enumerate(PC.SPECIAL_VALUES):
        p[idx[j::nv]] = val
    grad = torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    segs, off = [], 0
    for (r, c), gap in zip(SC.PLANES_SHAPES, SC.PLANES_GAPS):
        segs.append((off, r, c, torch.full((6 * r * c,), 0x7f, dtype=torch.uint8, device=DEV)))
        off += r * c + gap
    dp, dg, dm, dv = (t.to(DEV) for t in (p, grad, m, v))
    lr, wd, step = SC.PLANES_HYPER
    hip.adamw_planes(dp, dg, dm, dv, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step, segs)
    assert bool(torch.isfinite(dp).all()) and not torch.equal(dp.cpu(), p)
    for o, r, c, img in segs:
        want = words(hip.Planes(dp[o:o + r * c].view(r, c), True))
        assert torch.equal(img.view(torch.int16), want), (o, r, c, int((img.view(torch.int16) != want).sum()))


def test_packed_attention_planes_equal_the_split_pass_with_spread_values(hip):
    """mtvaf_prefix_attn_varlen_fwd_planes / _bwd_planes (test_packed_attention_writes_the_plane_images_of_its_results) with V -- the
    tokens' and the prefix's -- scaled per column by 2^[-30, 30]: context columns and dQ / dK spread over 60 binades, planes still
    those of the split pass over the fp32 results."""
    L_ = hip.lib()
    B, S, Pn, NH, p = 5, 100, 36, 4, 0.1
    H = NH * 64
    lens = [S, 1, 53, 20, 77]
    Mv = sum(lens)
    Mp = (Mv + 127) // 128 * 128 + 128
    scale = PC.per_exponent((H,), -30, 30, torch.Generator().manual_seed(70))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    q = rnd(Mv, 3 * H, seed=71)
    q[:, 2 * H:] *= scale
    qkv = torch.zeros(Mp, 3 * H, device=DEV)
    qkv[:Mv] = q.to(DEV)
    pk = rnd(B, Pn * H, seed=72).to(DEV)
    pv = (rnd(B, Pn, H, seed=73) * scale).reshape(B, Pn * H).contiguous().to(DEV)
    dctx = torch.zeros(Mp, H, device=DEV)
    dctx[:Mv] = rnd(Mv, H, seed=74).to(DEV)
    c1, l1 = nan(Mp, H), torch.zeros(B, NH, S, device=DEV)
    img = empty_image(hip, Mp, H)
    hip._ck(L_.mtvaf_prefix_attn_varlen_fwd_planes(hip._p(qkv), hip._p(pk), hip._p(pv), hip._p(cu), Mp - Mv, hip._p(c1), hip._p(l1), B, S, Pn, NH,
                                                   64, p, 11, 5, hip._p(img.img), Mp, hip._st()), "fwd planes")
    live = c1[:Mv].abs()
    assert bool(torch.isfinite(c1).all()) and float(live.max()) > 2.0 ** 20 and float(live[live != 0].min()) < 2.0 ** -20
    assert torch.equal(words(img), words(hip.Planes(c1, True)))
    d1 = nan(Mp, 3 * H)
    k1, v1 = torch.zeros(B, Pn * H, device=DEV), torch.zeros(B, Pn * H, device=DEV)
    de = torch.zeros(B, NH, S, device=DEV)
    dimg = empty_image(hip, Mp, 3 * H)
    hip._ck(L_.mtvaf_prefix_attn_varlen_bwd_planes(hip._p(dctx), hip._p(qkv), hip._p(pk), hip._p(pv), hip._p(cu), Mp - Mv, hip._p(c1), hip._p(l1),
                                                   hip._p(de), hip._p(d1), hip._p(k1), hip._p(v1), B, S, Pn, NH, 64, p, 11, 5, hip._p(dimg.img), Mp,
                                                   hip._st()), "bwd planes")
    assert bool(torch.isfinite(d1).all()) and float(d1.abs().max()) > 2.0 ** 20
    assert torch.equal(words(dimg), words(hip.Planes(d1, True)))


# ---------------------------------------------------------------------------------------------------------------------
# c. products on adversarial operands, every kernel of the family
# ---------------------------------------------------------------------------------------------------------------------
def family(hip, tiles, case, shape):
    """Every path of the family on one problem: accuracy (check) of each path's 128 x 128 launch, bit equality of every other tile
    and image layout with it."""
    M, N, K = shape
    A, B, ref, mag, bound = problem(case, shape)
    e_pipe = (pipe_product(hip, A, B) - ref).abs() / mag
    ok = lambda out, label: check(out, ref, mag, bound, e_pipe, case, (case, shape, label))
    a, bt, b, at = A.to(DEV), B.t().contiguous().to(DEV), B.to(DEV), A.t().contiguous().to(DEV)
    P = lambda t: {blk: hip.Planes(t, blk) for blk in (True, False)}
    pa, pbt, pb, pat = P(a), P(bt), P(b), P(at)
    wide256, wide192 = N % 256 == 0, N % 192 == 0 and N % 256 != 0
    # forward: C = A . (B^T)^T, both operands k-contiguous
    fwd = tiles(NARROW, KEY, lambda: hip.gemm_planes(pa[True], pbt[True], nan(M, N)))
    ok(fwd, "forward")
    assert same_bits(tiles(NARROW, KEY, lambda: hip.gemm_planes(pa[False], pbt[False], nan(M, N))), fwd), "natural images"
    wide_key = KEY + KEY_WIDE + (KEY_192 if wide192 else 0)
    if wide256 or wide192:
        for blk in (True, False):
            assert same_bits(tiles(FWD | NEVER_NARROW, wide_key, lambda: hip.gemm_planes(pa[blk], pbt[blk], nan(M, N))), fwd), ("wide forward", blk)
    if K >= 64:
        sk = tiles(NARROW, KEY, lambda: hip.gemm_planes(pa[True], pbt[True], nan(M, N), splits=2), splits=2)
        ok(sk, "split-K")
        if wide256 or wide192:
            assert same_bits(tiles(FWD | NEVER_NARROW, wide_key, lambda: hip.gemm_planes(pa[True], pbt[True], nan(M, N), splits=2), splits=2),
                             sk), "wide split-K"
    # dX form: B [K][N], the reduction index is its row
    dx = tiles(NARROW, KEY + KEY_B_KM, lambda: hip.gemm_planes(pa[True], pb[False], nan(M, N), layout_b=hip.KM))
    ok(dx, "dX")
    assert same_bits(tiles(NARROW, KEY + KEY_B_KM, lambda: hip.gemm_planes(pa[True], pb[True], nan(M, N), layout_b=hip.KM)), dx), "dX, blocked B"
    if wide256:
        for blk in (True, False):
            assert same_bits(tiles(DX | NEVER_NARROW, KEY + KEY_B_KM + KEY_WIDE,
                                   lambda: hip.gemm_planes(pa[True], pb[blk], nan(M, N), layout_b=hip.KM)), dx), ("wide dX", blk)
    if K >= 64:
        ok(tiles(NARROW, KEY + KEY_B_KM, lambda: hip.gemm_planes(pa[True], pb[False], nan(M, N), layout_b=hip.KM, splits=2), splits=2),
           "dX split-K")
    # dW form: A [K][M] and B [K][N]
    dw_key = KEY + KEY_A_KM + KEY_B_KM
    dw = tiles(NARROW, dw_key, lambda: hip.gemm_planes(pat[False], pb[False], nan(M, N), layout_a=hip.KM, layout_b=hip.KM))
    ok(dw, "dW")
    assert same_bits(tiles(NARROW, dw_key, lambda: hip.gemm_planes(pat[True], pb[True], nan(M, N), layout_a=hip.KM, layout_b=hip.KM)),
                     dw), "dW, blocked images"
    if wide256:
        for blk in (True, False):
            assert same_bits(tiles(DW | NEVER_NARROW, dw_key + KEY_WIDE,
                                   lambda: hip.gemm_planes(pat[blk], pb[blk], nan(M, N), layout_a=hip.KM, layout_b=hip.KM)), dw), ("wide dW", blk)
    # the grouped weight-gradient launch, two products: C and its transpose B^T . A
    for blk in (False, True):
        o1, o2 = nan(M, N), nan(N, M)
        tiles(NARROW, dw_key + KEY_GROUP, lambda: hip.gemm_planes_dw_group([(pat[blk], pb[blk], o1), (pb[blk], pat[blk], o2)]))
        assert same_bits(o1, dw), ("grouped launch, first product", blk)
        if blk:
            assert same_bits(o2, first_t), "grouped launch, blocked images"
        else:
            first_t = o2
            check(o2, ref.t(), mag.t(), bound.t(), e_pipe.t(), case, (case, shape, "grouped launch, second product"))


@pytest.mark.parametrize("shape", PC.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", PC.X3_CASES)
def test_presplit_family_on_adversarial_operands(hip, tiles, case, shape):
    """The operands of test_gemm_f32_split_adversarial (tests/x3_cases.py) through mtvaf_gemm_f32p on the 128 x 128, 128 x 256 and
    128 x 192 tiles, the dX and dW forms from natural and tile-blocked images, the grouped weight-gradient launch and 2-way split-K,
    at the smallest shapes where these kernels take different paths: that test's bounds on every path, and the same bits wherever
    the header promises them.  The launch profiler confirms the tile that was asked for."""
    family(hip, tiles, case, shape)


# ---------------------------------------------------------------------------------------------------------------------
# d. the edge of the split's domain, non-finite operands
# ---------------------------------------------------------------------------------------------------------------------
def test_specials_stay_finite_and_zeros_contribute_nothing(hip, tiles):
    """`specials` (+-0, fp32 subnormals, 2^-126, +-the largest magnitude whose first plane is finite) through the whole family under
    the bound of (c); the row of A that is all +-0 gives exact zeros, and the row of B that only meets the +-0 column of A may hold
    anything finite without changing one bit of the result."""
    M, N, K = shape = PC.SHAPES[1]
    family(hip, tiles, "specials", shape)
    A, B = problem("specials", shape)[:2]
    pa = hip.Planes(A.to(DEV), True)
    B2 = B.clone()
    B2[PC.ZERO_K] = rnd(N, seed=8) * 2.0 ** 40
    for mask, key in ((NARROW, KEY), (FWD | NEVER_NARROW, KEY + KEY_WIDE)):
        o1 = tiles(mask, key, lambda: hip.gemm_planes(pa, hip.Planes(B.t().contiguous().to(DEV), True), nan(M, N)))
        o2 = tiles(mask, key, lambda: hip.gemm_planes(pa, hip.Planes(B2.t().contiguous().to(DEV), True), nan(M, N)))
        assert bool((o1[PC.ZERO_ROW] == 0).all()) and bool((o2[PC.ZERO_ROW] == 0).all())
        assert same_bits(o1, o2), mask


def presplit_paths(hip, tiles, A, B):
    """[(label, C)] of A . B through the 128 x 128 tile, the 128 x 256 tile, the dW form and the in-kernel split"""
    (M, K), N = A.shape, B.shape[1]
    a, bt, b, at = A.to(DEV), B.t().contiguous().to(DEV), B.to(DEV), A.t().contiguous().to(DEV)
    pa, pbt, pb, pat = hip.Planes(a, True), hip.Planes(bt, True), hip.Planes(b, True), hip.Planes(at, True)
    return [("narrow", tiles(NARROW, KEY, lambda: hip.gemm_planes(pa, pbt, nan(M, N)))),
            ("wide", tiles(FWD | NEVER_NARROW, KEY + KEY_WIDE, lambda: hip.gemm_planes(pa, pbt, nan(M, N)))),
            ("dW", tiles(NARROW, KEY + KEY_A_KM + KEY_B_KM, lambda: hip.gemm_planes(pat, pb, nan(M, N), layout_a=hip.KM, layout_b=hip.KM))),
            ("in-kernel split", hip.gemm(a, 0, bt, 0, nan(M, N), M, N, K, compute="fp32x3", cfg=5))]


def test_overflow_edge_is_non_finite_on_the_split_arithmetic_and_finite_on_the_pipe(hip, tiles):
    """Operands at or above 2^127 (2 - 2^-8) -- finite fp32 numbers -- round to an infinite first plane: every result they feed is
    non-finite on the split arithmetic, pre-split or split in the kernel, every other result keeps the bits it has without them, and
    the fp32 pipe stays finite.  The limit the headers and DESIGN 4.1 state, pinned."""
    M, N, K = shape = PC.SHAPES[1]
    A, B = PC.operands("overflow_edge", M, N, K, seed=31)
    hit = torch.zeros(M, dtype=torch.bool)
    clean = A.clone()
    for i, j, _ in PC.poison_positions("overflow_edge", M, N, K):
        hit[i] = True
        clean[i, j] = 1.0
    assert bool(torch.isfinite(pipe_product(hip, A, B)).all())
    for (label, got), (_, want) in zip(presplit_paths(hip, tiles, A, B), presplit_paths(hip, tiles, clean, B)):
        assert not bool(torch.isfinite(got[hit]).any()), label
        assert bool(torch.isfinite(got[~hit]).all()) and same_bits(got[~hit], want[~hit]), label


@pytest.mark.parametrize("case", ["nonfinite", "nonfinite_b"])
def test_non_finite_operands_reach_every_result_they_feed_and_no_other(hip, tiles, case):
    """One +inf, one -inf and one NaN in A (in B): every output row (column) they feed is non-finite, every other output is finite,
    within the bound of (c) and bit for bit what it is without them -- 128 x 128 tile, 128 x 256 tile, dW form, the in-kernel split,
    and mtvaf_gemm_f32p_ep in its fp32 result and in the planes it writes."""
    M, N, K = shape = PC.SHAPES[1]
    A, B = PC.operands(case, M, N, K, seed=41)
    clean_a, clean_b = A.clone(), B.clone()
    hit = torch.zeros(M if case == "nonfinite" else N, dtype=torch.bool)
    for i, j, _ in PC.poison_positions(case, M, N, K):
        if case == "nonfinite":
            hit[i], clean_a[i, j] = True, 0.0
        else:
            hit[j], clean_b[i, j] = True, 0.0
    assert int(hit.sum()) == 3
    sel = (lambda t: t[hit], lambda t: t[~hit]) if case == "nonfinite" else (lambda t: t[:, hit], lambda t: t[:, ~hit])
    ref = clean_a.double() @ clean_b.double()
    bound = PC.error_bound(case, clean_a, clean_b, K)

    def verdict(got, want, label):
        assert not bool(torch.isfinite(sel[0](got)).any()), label
        rest = sel[1](got)
        assert bool(torch.isfinite(rest).all()), label
        assert bool(((rest.double().cpu() - sel[1](ref)).abs() <= sel[1](bound)).all()), label
        assert same_bits(rest, sel[1](want)), label
    for (label, got), (_, want) in zip(presplit_paths(hip, tiles, A, B), presplit_paths(hip, tiles, clean_a, clean_b)):
        verdict(got, want, label)
    # the plane-image epilogue
    imgs = []
    for a_, b_ in ((A, B), (clean_a, clean_b)):
        pa, pbt = hip.Planes(a_.to(DEV), True), hip.Planes(b_.t().contiguous().to(DEV), True)
        im, out = empty_image(hip, M, N), nan(M, N)
        tiles(NARROW, KEY, lambda: hip.gemm_planes_ep(pa, pbt, im, out=out))
        imgs.append((PC.unlayout(words(im).cpu(), M, N, True), out))
    verdict(imgs[0][1], imgs[1][1], "plane-image epilogue, fp32 result")
    for plane_got, plane_want in zip(imgs[0][0], imgs[1][0]):
        assert not bool(torch.isfinite(sel[0](plane_got.view(torch.bfloat16).float())).any())
        assert torch.equal(sel[1](plane_got), sel[1](plane_want))


# ---------------------------------------------------------------------------------------------------------------------
# e. mtvaf_gemm_f32p_slabs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout_b", [0, 1], ids=["forward", "dX"])
@pytest.mark.parametrize("shape", [(128, 128, 64), (256, 384, 96)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_planes_slabs(hip, shape, layout_b):
    """mtvaf_gemm_f32p_slabs (the executor's Wo, FFN-2 and FFN-1 dX products in front of LayerNorm): unsplit it is mtvaf_gemm_f32p;
    split, it leaves the slabs [M][N] in the workspace, C untouched, and slab 0 + slab 1 + bias (+ the old value, last) in fp32 is
    the split-K result of mtvaf_gemm_f32p bit for bit.  A workspace too small is refused before anything is written."""
    M, N, K = shape
    A, B = PC.operands("elementwise_spread", M, N, K, seed=51)
    pa = hip.Planes(A.to(DEV), True)
    pb = hip.Planes((B if layout_b else B.t().contiguous()).to(DEV), True)
    bias, old = rnd(N, seed=52).to(DEV), rnd(M, N, seed=53).to(DEV)
    ws = nan(2 * M * N)
    for acc in (False, True):
        start = old.clone() if acc else nan(M, N)
        # one slab: the result goes to C
        want = hip.gemm_planes(pa, pb, start.clone(), bias=bias, accumulate=acc, layout_b=layout_b)
        c = start.clone()
        assert hip.gemm_planes_slabs(pa, pb, c, ws, bias=bias, accumulate=acc, splits=1, layout_b=layout_b) == 1
        assert same_bits(c, want) and bool(torch.isnan(ws).all()), acc
        # two slabs: C stays as it was
        want = hip.gemm_planes(pa, pb, start.clone(), bias=bias, accumulate=acc, splits=2, layout_b=layout_b)
        c = start.clone()
        assert hip.gemm_planes_slabs(pa, pb, c, ws, bias=bias, accumulate=acc, splits=2, layout_b=layout_b) == 2
        assert same_bits(c, start), acc
        slabs = ws.view(2, M, N)
        assert bool(torch.isfinite(slabs).all())
        total = (slabs[0] + slabs[1]) + bias
        assert torch.equal(total + old if acc else total, want), acc
        ws.fill_(float("nan"))
    c = nan(M, N)
    for small in (nan(2 * M * N - 4), None):
        with pytest.raises(RuntimeError, match="workspace too small"):
            hip.gemm_planes_slabs(pa, pb, c, small, bias=bias, splits=2, layout_b=layout_b)
        assert bool(torch.isnan(c).all()) and (small is None or bool(torch.isnan(small).all()))
