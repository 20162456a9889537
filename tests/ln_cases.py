"""Case tables, input builders and plain float64 references of the row kernels of csrc/rowops.hip between attention and the
streaming kernels: ln_fwd_kernel<0/1/2, PL>, ln_bwd_kernel<0/1, PL>, ln_bwd_lean_kernel<PL, NS>, the deterministic embedding
scatter (row_nonzero -> det_count -> det_scan -> det_fill -> embed_scatter_det_kernel), its atomic fallback, pos_reduce_kernel and
roberta_pos_kernel.  Shared by test_ln_cases.py (CPU: proves the references and the bounds) and test_ln_kernels_gpu.py (the
kernels).  Nothing here imports mtvaf_amd: the references are torch on the host, in float64 from the fp32 inputs.

Every case is the smallest shape that reaches its branch; the ids name the branch a case is there for.  Dropout enters every
reference as an explicit keep tensor (0 or float32(1 / (1 - p))): the GPU test obtains it from hip.dropout(ones, ...) at the same
(seed, offset) -- row * (H / 4) + chunk is the flat float4 index of dropout_kernel for a contiguous [M, H] tensor."""
import torch

from stream_cases import SENTINEL, close_excess, dropout_scale, gen, guard_mask, norm_excess, ulp32, view_layout  # noqa: F401

U32 = 2.0 ** -24  # unit roundoff of fp32

# the caps the M values below cross, restated (csrc/rowops.hip: row_grid, row_grid_bwd, mtvaf_dropout_res_ln_bwd_finish)
FWD_GRID_ROWS = 1024 * 4      # row_grid: 1024 blocks x 4 rows per trip
BWD_GRID_ROWS = 512 * 4       # row_grid_bwd, wave-per-row kernel: 512 blocks x 4 rows per trip
LEAN_GRID_ROWS = 512          # row_grid_bwd, lean kernel: one row per block and trip
FINISH_WIDE_BLOCKS = 128      # _bwd_finish: colsum_final_multi_kernel<32> from 128 partial rows, <8> below
MAX_H = 1024
SCAN_MAX_VOCAB = 65536        # det_scan_kernel: MAXQ = 16 int4 vectors x 1024 threads; above: the atomic scatter


def bwd_blocks(M):
    return max(1, min((M + 3) // 4, 512))


def lean_shape(H):
    """ln_lean: H % 256 == 0 (block of H / 4 threads: 1 to 4 waves); every other H takes the wave-per-row kernel"""
    return H % 256 == 0 and H <= MAX_H


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
# inherited (test_ops_gpu.py `close`): rows (y, dx, dres, dz) and column sums (dgamma, dbeta, dbias_x, dword, dpos, dtype)
RTOL_ROW, RTOL_COL = 2e-4, 5e-4
# Derived, for what `close` cannot hold or never bounded.  The kernels keep z = x * keep + res in fp32 registers and take
#   mu = fl(sum z / H), d = fl(z - mu), var = fl(sum d^2 / H), rstd = rsqrt(var + eps), xh = d * rstd.
#  * mean: a sum of H <= 1024 terms in 16 in-lane additions and 6 shuffle levels, one division, one store: each addition rounds
#    at <= U32 * |partial sum| <= U32 * H * max|z| / (the division by H) -> |d mu| <= ~(22 + 2) * U32 * max|z| in the worst
#    case and a few U32 * max|z| for random signs.  MEAN_K * U32 * max_row|z| with MEAN_K = 8.
#  * xh: d inherits d mu (the subtraction itself is exact or rounds at ulp(d)), so |d xh| <= MEAN_K * U32 * A with
#    A = max_row|z| * rstd, the row's condition (>= 1; 1e3 for a common offset of 1e3 at sigma 1).  Storing mean in fp32 alone
#    costs ulp(|mean|) * rstd = 6e-5 in y at an offset of 1e3 (1.2e-4 measured for a plain fp32 two-pass statement, 1.2e-3 at
#    1e4: the bound scales with A, and 1e3 is the largest offset kept as a random case).  K_COND = 16 = 2 * MEAN_K: the
#    constant of every term below that carries d xh.
#  * rstd: z = fl(x * keep + res) is itself rounded at <= U32 * |z| per element before the statistics see it: to first order
#    var moves by 2 * mean(d * dz) <= 2 * sigma * U32 * max|z|, i.e. by 2 * U32 * A of itself, and rstd by U32 * A (twice that
#    is allowed: the product x * keep rounds too).  An error e of the mean enters at second order only -- sum (d - e)^2 =
#    sum d^2 + H e^2 because sum d = 0 -- and rsqrt is off by <= 2 ulp behind a few roundings of the sum: relative
#    RSTD_K * U32 + 2 * U32 * A + (MEAN_K * U32 * A)^2 with RSTD_K = 16.
#  * y = xh * gamma + beta: `close` + K_COND * U32 * A * |gamma_c|.
#  * dz = (g - m1 - xh * m2) * rstd with g = dy * gamma, m1 = mean g, m2 = mean(g * xh), |m2| <= max|g|:
#    `close` + K_COND * U32 * A * rstd * max_row|g| (times the keep factor for dx).
#  * dgamma_c = sum_r dy_rc xh_rc: `close` + K_COND * U32 * sum_r A_r |dy_rc|;  dbias_x_c = sum_r dx_rc: `close` + sum_r of
#    the dx term;  dbeta = sum dy does not see the statistics: `close` alone.
# The derived terms are added for the input kinds in COND_KINDS only; everywhere else the inherited bound stands alone.
MEAN_K, RSTD_K, K_COND = 8.0, 16.0, 16.0
COND_KINDS = ("offset1e3", "one-outlier", "eps-dominates", "tiny-1e-20", "huge-1e15")


def excess(got, ref, rtol, extra=None):
    """max over the elements of err / allowed (<= 1 passes).  allowed = the `close` of test_ops_gpu.py (atol = rtol * max|ref| +
    1e-7) with the constant 1e-7 capped at rtol * max|ref| -- so that a tensor of the order of 1e-15 is not compared against
    1e-7: never wider than `close` -- plus the derived term `extra` (float64, broadcastable) where a case has one."""
    ref32 = ref.detach().float().cpu().double()
    top = rtol * float(ref32.abs().max()) if ref32.numel() else 0.0
    if extra is None and top >= 1e-7:
        return close_excess(got, ref, rtol)
    got = got.detach().float().cpu().double()
    allowed = top + min(1e-7, top) + rtol * ref32.abs()
    if extra is not None:
        allowed = allowed + extra
    err = (got - ref32).abs()
    bad = err > allowed
    if not bool(bad.any()):
        return float((err / allowed.clamp_min(1e-300)).max()) if err.numel() else 0.0
    return float((err[bad] / allowed.expand_as(err)[bad].clamp_min(1e-300)).max())


def mean_excess(got, ref_mean, z):
    bound = MEAN_K * U32 * z.double().abs().amax(-1)
    err = (got.detach().cpu().double() - ref_mean).abs()
    return float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0


def rstd_excess(got, ref_rstd, z):
    A = z.double().abs().amax(-1) * ref_rstd
    bound = (RSTD_K * U32 + 2 * U32 * A + (MEAN_K * U32 * A) ** 2) * ref_rstd
    return float(((got.detach().cpu().double() - ref_rstd).abs() / bound).max())


def cond_terms(z, rstd, gamma, dy, keep=None):
    """the derived terms of a COND_KINDS case (float64): dict y, dx (= dres, dz), dgamma, dbias_x"""
    z, rstd, gamma, dy = z.double(), rstd.double(), gamma.double(), dy.double()
    A = z.abs().amax(-1) * rstd
    g = (dy * gamma).abs().amax(-1)
    dx = (K_COND * U32 * A * rstd * g)[:, None]
    if keep is not None:
        dx = dx * keep.double().amax()
    return {"y": K_COND * U32 * A[:, None] * gamma.abs()[None, :], "dx": dx,
            "dgamma": K_COND * U32 * (A[:, None] * dy.abs()).sum(0), "dbias_x": dx.sum(0).expand(z.shape[1])}


# ---------------------------------------------------------------------------------------------------------------------
# references (dtype float64) and their plain fp32 restatement (dtype float32: the same lines, every operation rounded)
# ---------------------------------------------------------------------------------------------------------------------
def ln_ref(z, gamma, beta, eps, dtype=torch.float64):
    """-> y, mean, rstd of LayerNorm over the last axis (biased variance, two passes)"""
    z, gamma, beta = z.to(dtype), gamma.to(dtype), beta.to(dtype)
    H = z.shape[-1]
    mean = z.sum(-1) / H
    d = z - mean[:, None]
    rstd = 1.0 / ((d * d).sum(-1) / H + torch.tensor(eps, dtype=dtype)).sqrt()
    return d * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd_ref(dy, z, gamma, mean, rstd, dtype=torch.float64):
    """-> dz, dgamma, dbeta for upstream dy of y = LN(z) * gamma + beta"""
    dy, z, gamma = dy.to(dtype), z.to(dtype), gamma.to(dtype)
    H = z.shape[-1]
    xh = (z - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    g = dy * gamma
    m1, m2 = g.sum(-1) / H, (g * xh).sum(-1) / H
    dz = (g - m1[:, None] - xh * m2[:, None]) * rstd.to(dtype)[:, None]
    return dz, (dy * xh).sum(0), dy.sum(0)


def res_ln_ref(x, res, gamma, beta, eps, keep=None, dtype=torch.float64):
    """z = x * keep + res; -> y, mean, rstd, z"""
    z = x.to(dtype) * (keep.to(dtype) if keep is not None else 1.0) + res.to(dtype)
    return ln_ref(z, gamma, beta, eps, dtype) + (z,)


def res_ln_bwd_ref(dout, x, res, gamma, eps, keep=None, dtype=torch.float64, stats=None):
    """-> dx, dres, dgamma, dbeta, dbias_x (the column sums of dx).  stats = (mean, rstd) to take instead of recomputing them."""
    z = x.to(dtype) * (keep.to(dtype) if keep is not None else 1.0) + res.to(dtype)
    _, mean, rstd = ln_ref(z, gamma, torch.zeros_like(gamma), eps, dtype)
    if stats is not None:
        mean, rstd = stats
    dz, dgamma, dbeta = ln_bwd_ref(dout, z, gamma, mean, rstd, dtype)
    dx = dz * keep.to(dtype) if keep is not None else dz
    return dx, dz, dgamma, dbeta, dx.sum(0)


def embed_gather_ref(ids, tts, pos_ids, word, pos, typ, dtype=torch.float64):
    """word[id] + type[tt] + pos[p], p = arange(S) (BERT) or the explicit position ids (RoBERTa) -> [B * S, H]"""
    B, S = ids.shape
    p = pos_ids.long() if pos_ids is not None else torch.arange(S)[None, :].expand(B, S)
    z = word.to(dtype)[ids] + typ.to(dtype)[tts] + pos.to(dtype)[p]
    return z.reshape(B * S, -1)


def embed_ln_ref(ids, tts, pos_ids, word, pos, typ, gamma, beta, eps, keep=None, dtype=torch.float64):
    """-> out = dropout(LN(z)), mean, rstd, z"""
    z = embed_gather_ref(ids, tts, pos_ids, word, pos, typ, dtype)
    y, mean, rstd = ln_ref(z, gamma, beta, eps, dtype)
    return (y * keep.to(dtype) if keep is not None else y), mean, rstd, z


def embed_ln_bwd_ref(dout, ids, tts, pos_ids, word, pos, typ, gamma, eps, word_pad, pos_pad, keep=None, prev=None,
                     dtype=torch.float64):
    """-> dz, dword, dpos, dtype, dgamma, dbeta.  The table gradients are an index_add_ over the tokens: none for word_pad rows,
    none for pos_pad rows when position ids are given; prev = (dword, dpos, dtype, dgamma, dbeta) to accumulate onto."""
    B, S = ids.shape
    z = embed_gather_ref(ids, tts, pos_ids, word, pos, typ, dtype)
    _, mean, rstd = ln_ref(z, gamma, torch.zeros_like(gamma), eps, dtype)
    dy = dout.to(dtype) * (keep.to(dtype) if keep is not None else 1.0)
    dz, dgamma, dbeta = ln_bwd_ref(dy, z, gamma, mean, rstd, dtype)
    fid, ftt = ids.reshape(-1), tts.reshape(-1)
    dword, dpos, dtyp = (torch.zeros(t.shape, dtype=dtype) for t in (word, pos, typ))
    m = fid != word_pad
    dword.index_add_(0, fid[m], dz[m])
    if pos_ids is None:
        dpos.index_add_(0, torch.arange(S).repeat(B), dz)
    else:
        fp = pos_ids.reshape(-1).long()
        m = fp != pos_pad
        dpos.index_add_(0, fp[m], dz[m])
    dtyp.index_add_(0, ftt, dz)
    outs = [dword, dpos, dtyp, dgamma, dbeta]
    if prev is not None:
        outs = [o + p.to(dtype) for o, p in zip(outs, prev)]
    return (dz,) + tuple(outs)


def roberta_pos_ref(ids, pad):
    """cumsum(ids != pad) * (ids != pad) + pad, as a loop -> int64 [B, S]"""
    B, S = ids.shape
    out = torch.empty(B, S, dtype=torch.int64)
    for b in range(B):
        run = 0
        for s in range(S):
            if int(ids[b, s]) != pad:
                run += 1
                out[b, s] = run + pad
            else:
                out[b, s] = pad
    return out


# ---------------------------------------------------------------------------------------------------------------------
# residual LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
LN_H = {4: "one-lane", 8: "partial-first-chunk", 252: "last-lane-masked", 256: "one-chunk-lean-one-wave", 260: "chunk2-four-lanes",
        512: "lean-two-waves", 768: "lean-three-waves", 1020: "last-chunk-partial", 1024: "lean-four-waves-all-chunks-full"}
LN_SMALL_M = [1, 3, 4, 5]  # waves of a block without a row
# (M, H, why)
LN_BIG = [(4097, 8, "second-forward-stride-trip"), (4097, 256, "second-forward-stride-trip-lean"),
          (2049, 8, "second-backward-trip-wave-per-row"), (2049, 256, "second-backward-trip-lean"),
          (508, 8, "finish-127-partial-rows-8-groups"), (509, 8, "finish-128-partial-rows-32-groups")]
LN_SHAPES = [(M, H, LN_H[H]) for H in LN_H for M in LN_SMALL_M] + LN_BIG
LN_P = 0.1  # the shape cases run with dropout: masks and scale take part in every one of them


def ln_shape_id(c):
    return "M{}-H{}-{}".format(*c)


LN_KINDS = ["unit", "offset1e3", "constant-row", "eps-dominates", "tiny-1e-20", "huge-1e15", "one-outlier", "gamma0-beta1"]
KIND_SHAPES = [(5, 8), (5, 260), (5, 768)]  # wave-per-row with one chunk, with two, lean
# constants whose sums over <= 1024 terms are exact in fp32 in any order: the kernels' variance of such a row is exactly 0
CONSTANTS = [0.5, -3.0, 2.0, -0.25, 1.0]
# scales of the tiny / huge kinds as the issue states them: the float64 reference stays inside fp32 range at both (huge: the
# squares sum to <= 1024 * (5e15)^2 = 2.6e34 < 3.4e38, dx ~ 1e-15; tiny: d^2 ~ 1e-40 is a denormal beside eps = 1e-12)
TINY, HUGE = 1e-20, 1e15


def ln_inputs(M, H, kind, seed=0):
    """-> x, res, gamma, beta, dout (fp32), eps"""
    g = gen(1000 * M + H + seed)
    x, res = torch.randn(M, H, generator=g), torch.randn(M, H, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    dout = torch.randn(M, H, generator=g)
    eps = 1e-12
    if kind == "offset1e3":  # every element of a row shares +-1e3, sigma 1
        sign = torch.tensor([1.0 if r % 2 == 0 else -1.0 for r in range(M)])
        x = (1e3 * sign)[:, None].expand(M, H).contiguous()
    elif kind == "constant-row":
        c = torch.tensor([CONSTANTS[r % len(CONSTANTS)] for r in range(M)])
        x = (c / 2)[:, None].expand(M, H).contiguous()
        res = x.clone()
        eps = 1e-5
    elif kind == "eps-dominates":  # sigma(z) = 1e-4, eps = 1e-5 >> var = 1e-8
        x, res = x * (1e-4 / 2 ** 0.5), res * (1e-4 / 2 ** 0.5)
        eps = 1e-5
    elif kind == "tiny-1e-20":
        x, res = x * TINY, res * TINY
    elif kind == "huge-1e15":
        x, res = x * HUGE, res * HUGE
    elif kind == "one-outlier":  # one element 1e4 among unit noise
        for r in range(M):
            x[r, (7 * r + 1) % H] = 1e4
            res[r, (7 * r + 1) % H] = 0.0
    elif kind == "gamma0-beta1":
        gamma, beta = torch.zeros(H), torch.ones(H)
    else:
        assert kind == "unit", kind
    return x, res, gamma, beta, dout, eps


# entry-point variants, each at one wave-per-row and the lean block sizes: (M, H)
VARIANT_SHAPES = [(5, 32), (5, 260), (5, 256), (3, 512), (5, 768), (4, 1024)]
PLANE_SHAPES = [(5, 32), (5, 256)]  # H % 32 == 0: wave-per-row and lean
SLAB_COUNTS = [1, 2, 3]             # NS = 1, 2, -1 of the lean kernel


def slab_inputs(M, H, nslab, seed=0):
    """-> slabs [nslab, M, H], bias [H]"""
    g = gen(77 * M + H + nslab + seed)
    return torch.randn(nslab, M, H, generator=g), torch.randn(H, generator=g)


def slab_sum(slabs, bias=None, dtype=torch.float64):
    """slab 0 + slab 1 + ... (+ bias), in the kernels' order"""
    s = slabs[0].to(dtype)
    for k in range(1, slabs.shape[0]):
        s = s + slabs[k].to(dtype)
    return s + bias.to(dtype) if bias is not None else s


# ---------------------------------------------------------------------------------------------------------------------
# embeddings
# ---------------------------------------------------------------------------------------------------------------------
REPEAT = 7  # the id whose segment a case sizes
# fields: n = rows of REPEAT (interleaved with distinct other ids: S = n, B = 2), H, vocab, type_vocab, roberta, zero = which
# dout rows are exactly zero, acc, p, pad = word (and RoBERTa position) padding id, extra_pos = max_pos - what S needs
EMBED_DEFAULT = dict(n=5, H=8, vocab=300, type_vocab=2, roberta=False, zero="none", acc=0, p=0.0, pad=0, extra_pos=3, top_id=False,
                     pad_hits=False)


def _ec(cid, **kw):
    d = dict(EMBED_DEFAULT, id=cid)
    d.update(kw)
    return d


SEG_N = {1: "single-row", 2: "half-group", 3: "group-less-one", 4: "one-group", 5: "group-plus-one", 63: "register-ranked-ragged",
         64: "last-register-ranked", 65: "long-branch-first-trip", 67: "long-branch-ragged-tail", 130: "long-branch-third-trip"}
EMBED_CASES = [_ec("seg-n%d-%s" % (n, why), n=n) for n, why in SEG_N.items()] + [
    _ec("seg-n67-zero-rows-skipped-owner-moves", n=67, zero="some"),
    _ec("seg-n5-zero-rows-skipped-owner-moves", n=5, zero="some"),
    _ec("all-rows-zero", n=5, zero="all"),
    _ec("word-pad-ids", n=6, pad_hits=True),
    _ec("roberta-pos-pad-rows-explicit-position-ids", n=6, roberta=True, pad=1, pad_hits=True, type_vocab=1),
    _ec("roberta-n65-long-word-segment-both-keys", n=65, roberta=True, pad=1, pad_hits=True, type_vocab=1),
    _ec("bert-max-pos-gt-S-accumulate-rows-above-S-untouched", n=5, acc=1, extra_pos=6),
    _ec("roberta-accumulate", n=6, roberta=True, pad=1, pad_hits=True, acc=1),
    _ec("type-vocab1", n=4, type_vocab=1),
    _ec("type-vocab1-accumulate", n=4, type_vocab=1, acc=1),
] + [_ec("vocab%d-top-id-%s" % (v, why), n=3, vocab=v, top_id=True)
     for v, why in ((4095, "scan-share-4-last-short"), (4096, "scan-share-4-full"), (4097, "scan-share-8"),
                    (65536, "scan-share-64-MAXQ16"))] + [
    _ec("H%d-n%d" % (H, n), n=n, H=H) for H in (4, 260, 1024) for n in (5, 65)] + [
    _ec("dropout-p%g" % p, n=5, p=p, H=260) for p in (0.1, 0.5)]
EMBED_ATOMIC_CASE = _ec("vocab65537-atomic-fallback", n=5, vocab=65537, top_id=True)
EMBED_TWICE_CASE = EMBED_CASES[9]   # n = 130: deterministic mode twice, torch.equal
EMBED_MODE_CASE = EMBED_CASES[8]    # n = 67: mtvaf_embed_scatter_mode(1) against mode 0
EMBED_SEED, EMBED_OFFSET = 41, 9


def embed_inputs(c):
    """-> dict: ids [B, S] int64, tts, pos_ids (int32 or None), word / pos / typ tables, gamma, beta, dout [B * S, H], prev (the
    five prior contents for the accumulating form), B, S, max_pos, eps, word_pad, pos_pad, rep_rows (the rows of REPEAT)"""
    n, H, vocab = c["n"], c["H"], c["vocab"]
    B, S = 2, n
    M = B * S
    g = gen(n * 131 + H + vocab)
    pad = c["pad"]
    # REPEAT on the even rows, distinct other ids (neither REPEAT nor pad) on the odd ones: the segment is not contiguous
    others = [i for i in range(2, 2 + n + 8) if i not in (REPEAT, pad)][:n]
    flat = torch.empty(M, dtype=torch.int64)
    flat[0::2] = REPEAT
    flat[1::2] = torch.tensor(others)
    if c["top_id"]:
        flat[1] = vocab - 1
    if c["pad_hits"]:  # the padding id on an odd row in the middle and at the tail
        flat[M // 2 | 1] = pad
        flat[M - 1] = pad
    ids = flat.view(B, S)
    tv = c["type_vocab"]
    tts = (torch.arange(M) % 3 == 1).long().view(B, S) if tv > 1 else torch.zeros(B, S, dtype=torch.int64)
    pos_ids = None
    max_pos = S + c["extra_pos"]
    if c["roberta"]:
        pos_ids = roberta_pos_ref(ids, pad).to(torch.int32)
        max_pos = S + pad + 1 + c["extra_pos"]
    word, pos, typ = (torch.randn(r, H, generator=g) for r in (vocab, max_pos, tv))
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    dout = torch.randn(M, H, generator=g)
    rep_rows = torch.arange(0, M, 2)
    if c["zero"] == "some":  # the segment's smallest row (ownership moves), one in the middle, the last, and a foreign row
        zr = [0, int(rep_rows[n // 2]), int(rep_rows[-1]), 1]
        dout[zr] = 0.0
    elif c["zero"] == "all":
        dout.zero_()
    pat = lambda t, k: (torch.arange(t.numel(), dtype=torch.float32).view(t.shape) % 13 - 6) * 0.25 + k
    prev = (pat(word, 1), pat(pos, 2), pat(typ, 3), pat(gamma, 4), pat(beta, 5))
    return dict(ids=ids, tts=tts, pos_ids=pos_ids, word=word, pos=pos, typ=typ, gamma=gamma, beta=beta, dout=dout, prev=prev,
                B=B, S=S, max_pos=max_pos, eps=1e-12, word_pad=pad, pos_pad=pad if c["roberta"] else -1, rep_rows=rep_rows)


# ---------------------------------------------------------------------------------------------------------------------
# RoBERTa position ids
# ---------------------------------------------------------------------------------------------------------------------
POS_S = [1, 63, 64, 65, 128, 129, 200]
POS_PATTERNS = ["no-padding", "all-padding", "padding-at-the-tail", "padding-at-position-0", "padding-across-the-64-token-trips"]
POS_PAD = 1


def pos_ids_inputs(S):
    """-> ids int64 [len(POS_PATTERNS), S], one pattern per row"""
    g = gen(S)
    ids = torch.randint(2, 100, (len(POS_PATTERNS), S), generator=g)
    ids[1] = POS_PAD
    ids[2, S - (S + 2) // 3:] = POS_PAD
    ids[3, 0] = POS_PAD
    for s in (5, 62, 63, 64, 65, 100, 126, 127, 128, 129, 191, 192):
        if s < S:
            ids[4, s] = POS_PAD
    return ids


# ---------------------------------------------------------------------------------------------------------------------
# the exact cross-kernel contract: every dropout site scales kept elements by float32(1 / (1 - p)), as mtvaf_dropout
# ---------------------------------------------------------------------------------------------------------------------
EXACT_PS = [0.1, 0.5, 0.9]
EXACT_SHAPES = [(6, 8), (5, 260), (5, 256), (3, 1024)]  # wave-per-row (two of them), lean one wave, lean four waves
EXACT_SEED, EXACT_OFFSET = 1234, 5


def exact_bwd_inputs(M, H):
    """MODE 0 backward whose dz is exactly +-1 before the keep factor: x = res = 0 with mean = 0, rstd = 1 handed in (xh = 0),
    gamma = 1, dout alternating +-1 along the row (m1 = 0 exactly: H is even) -> dz = (dout - 0 - 0 * m2) * 1
    -> x, res, gamma, mean, rstd, dout"""
    dout = torch.ones(M, H)
    dout[:, 1::2] = -1.0
    return torch.zeros(M, H), torch.zeros(M, H), torch.ones(H), torch.zeros(M), torch.ones(M), dout
