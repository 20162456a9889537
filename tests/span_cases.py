"""Case tables, input builders and plain float64 references of the span-model heads of csrc/span.hip: span_index_kernel,
span_pool_fwd_kernel, span_pool_bwd_span_kernel / span_pool_bwd_token_kernel, distant_ce_fwd / mean / bwd, ce_fwd / bwd and
mask_mul_kernel.  Shared by test_span_cases.py (CPU: proves the references and the bounds) and test_span_kernels_gpu.py (the
kernels).  Nothing here imports mtvaf_amd: the references are torch on the host, in float64 from the fp32 inputs.

Every case is the smallest shape that reaches its branch; the ids name the branch a case is there for.  Every input is inside the
contract of include/mtvaf_hip.h: labels in [0, C) or -100, span starts >= 0, sizes the entry points accept.

Worst excess (error / bound) measured on the MI355X with the shift-safe loss kernels stands beside the bound it belongs to
below.  The kernels before that change (sum pos z against den lse; m + log e - z_label) failed the eight offset +-1e4 cases and no
other: distant-CE loss 4.89 and dlogits 1.78 (B2-S65), 2.81 and 1.17 (B3-S130); CE loss 3.48 and ws2 3.58 (N33-C4), 1.49 and 1.51
(N5-C64).  At +-1e3 they stayed inside the inherited tolerances (distant-CE loss 0.24, dlogits 0.08; CE loss 0.08)."""
import torch
import torch.nn.functional as F

from ln_cases import U32, excess  # noqa: F401
from oracle import mtvaf_oracle as O
from stream_cases import SENTINEL, close_excess, gen, guard_mask, ulp32, view_layout  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
# inherited (test_span_gpu.py): `close` rtol of pooled, of dseq and dw, of both dlogits; the losses |err| <= 1e-5 |ref| + 1e-6
RTOL_POOLED, RTOL_POOL_GRAD, RTOL_DLOGITS = 1e-4, 1e-3, 1e-4      # GPU worst: pooled 0.0008, dseq 0.0015, dw 0.0036; dlogits 0.0010 (distant CE), 0.0011 (CE)
LOSS_RTOL, LOSS_ATOL = 1e-5, 1e-6                                 # GPU worst: distant-CE loss 0.012, CE loss 0.013, ws2 0.010
# Derived, for what the inherited bounds cannot hold or never bounded.
#  * a dot product over H <= 1024 elements is 16 in-lane multiply-adds and 6 shuffle levels: each rounds at <= U32 * |partial|,
#    in the worst case 22 * U32 * sum|a_h b_h| and a few U32 of that for random signs -- DOT_K = 8, the MEAN_K of ln_cases.py.
#  * db: the score bias shifts every score of a span alike and the softmax does not see a shift: db = sum_n sum_r ds_nr with
#    ds_nr = p_nr (g_n . x_r - g_n . o_n) is 0 in exact arithmetic, and what a kernel returns is the rounding of the two dot
#    products: |db| <= DOT_K * U32 * sum_nr p_nr (sum_h |g_nh x_rh| + sum_h |g_nh o_nh|) ;  the additions of the sum
#    itself round at U32 * |ds|, below that).                                                    GPU worst: 0.105
#  * ill-conditioned scores (POOL_COND_KINDS): a score x_r . w + b (+ -10000 behind the span) is off by
#    delta_n = DOT_K * U32 * max_r (sum_h |x_rh w_h| + |b| + 10000 [r >= width]), which is ulp-sized against the score, not
#    against 1: 3e-5 at |score| 50, 1e-2 at 2e4.  To first order d p_r = p_r (d sc_r - sum_r' p_r' d sc_r'), |d p_r| <= 2 delta p_r,
#    and sum_r d p_r = 0, so with dev_r = x_r - o:
#      pooled:  |d o_h| <= 2 delta sum_r p_r |dev_rh|
#      ds_r = p_r g . dev_r:  |d ds_r| <= 2 delta p_r (|g . dev_r| + G),  G = sum_r' p_r' |g . dev_r'| >= |g . d o| / (2 delta)
#    and, ds being tiny where the softmax is one-hot, the db term of the two dot products on top of it (|d ds_r| is their sum);
#      dw_h = sum_nr ds_nr x_rh:  sum_nr |d ds_nr| |x_rh|;   db: sum_nr |d ds_nr|
#      dseq[row] = sum over the (n, r) that read the row of p_nr g_n + ds_nr w:  sum of 2 delta p_nr |g_n| + |d ds_nr| |w|
#    The terms vanish with the spread of a span's rows around its pooled value: a near one-hot softmax gets almost nothing.
#  * CE: the kernel adds the N row losses one after the other: rounding k is at most U32 * (partial sum k), the partial sums of
#    positive terms grow linearly to the total: (N - 1) / 2 * U32 * |loss| (`ce_sum_term`; 1.9e-5 relative at N = 640, under
#    the inherited 1e-5 up to N = 300).
DOT_K = 8.0
POOL_COND_KINDS = ("onehot50", "addmask2e4")
MASKED = -10000.0  # the additive mask of the reference (not -inf: a masked position far ahead keeps its weight)


def loss_excess(got, ref, extra=0.0):
    """|got - ref| / (1e-5 |ref| + 1e-6 + extra); NaN where exactly one of the two is NaN"""
    got, ref = (float(t.detach()) if torch.is_tensor(t) else float(t) for t in (got, ref))
    if ref != ref or got != got:
        return 0.0 if (ref != ref and got != got) else float("nan")
    return abs(got - ref) / (LOSS_RTOL * abs(ref) + LOSS_ATOL + extra)


def ce_sum_term(N, ref):
    return 0.5 * (N - 1) * U32 * abs(float(ref))


# ---------------------------------------------------------------------------------------------------------------------
# span_index
# ---------------------------------------------------------------------------------------------------------------------
INDEX_THREADS = 1024  # span_index_kernel: one block; tokens in chunks of ceil(B S / 1024), spans in a stride loop


def _ic(cid, B, S, M, mask="ragged", spans="plain"):
    return dict(id=cid, B=B, S=S, M=M, mask=mask, spans=spans)


INDEX_CASES = [
    _ic("B3-S343-M2-chunk2-sentences-start-mid-chunk", 3, 343, 2),
    _ic("B35-S4-M30-span-loop-second-trip", 35, 4, 30),
    _ic("B3-S7-M3-masked-sentence-between-live-ones", 3, 7, 3, mask="middle-empty"),
    _ic("B3-S12-M4-holes", 3, 12, 4, mask="holes"),
    _ic("B2-S5-M2-T0-all-masked", 2, 5, 2, mask="none"),
    _ic("B2-S5-M2-T1", 2, 5, 2, mask="one"),
    _ic("B2-S6-M3-all-widths-nonpositive-JR0", 2, 6, 3, spans="empty"),
    _ic("B2-S6-M3-one-span-wider-than-S-JR-clamped", 2, 6, 3, spans="wider-than-S"),
]


def span_mask(B, S, kind, g):
    """-> uint8 [B, S]"""
    if kind == "none":
        return torch.zeros(B, S, dtype=torch.uint8)
    if kind == "one":
        m = torch.zeros(B, S, dtype=torch.uint8)
        m[B - 1, 1] = 1
        return m
    lens = torch.randint(min(3, S), S + 1, (B,), generator=g)
    lens[0] = S
    m = (torch.arange(S)[None, :] < lens[:, None]).to(torch.uint8)
    if kind == "full":
        m[:] = 1
    elif kind == "middle-empty":
        m[B // 2] = 0
    elif kind == "holes":
        m[1 % B, 1] = 0
        m[2 % B, 0] = 0
        m[0, S // 2] = 0
    else:
        assert kind == "ragged", kind
    return m


def span_bounds(mask, M, kind, g):
    """-> starts, ends int64 [B, M]: 0 <= start < max(len, 1), start <= end <= start + 3 inside the sentence ("plain")"""
    B, S = mask.shape
    lens = mask.ne(0).sum(-1).clamp_min(1)
    starts = (torch.rand(B, M, generator=g) * lens[:, None]).long()
    ends = torch.minimum(starts + torch.randint(0, 4, (B, M), generator=g), (lens - 1)[:, None].expand(B, M)).long()
    ends = torch.maximum(ends, starts)
    if kind == "empty":            # end < start everywhere: every width <= 0
        ends = starts - 1 - torch.randint(0, 2, (B, M), generator=g)
    elif kind == "wider-than-S":   # width S + 3
        starts[0, 1], ends[0, 1] = 1, 1 + S + 2
    elif kind == "pile-on-last":   # a wide span sets JR; the last sentence's spans start on its last tokens and are clipped
        starts[0, 0], ends[0, 0] = 0, min(S, 5) - 1
        last = int(lens[B - 1]) - 1
        starts[B - 1, :] = torch.tensor([max(last - (m % 2), 0) for m in range(M)])
        ends[B - 1, :] = starts[B - 1, :]
    elif kind == "cover-one-token":  # every span reads flat token 1 and none reads beyond flat token 3
        starts = (torch.arange(B * M).view(B, M) % 2).long()
        ends = 1 + (torch.arange(B * M).view(B, M) // 2 % 2).long()
    else:
        assert kind == "plain", kind
    return starts, ends


def index_inputs(c):
    g = gen(7 * c["B"] + 13 * c["S"] + c["M"])
    mask = span_mask(c["B"], c["S"], c["mask"], g)
    starts, ends = span_bounds(mask, c["M"], c["spans"], g)
    return mask, starts, ends


def span_geometry(mask, starts, ends):
    """-> rowmap [T] (b * S + s of the live tokens in order), woff [B], soff [B * M], width [B * M], T, JR"""
    B, S = mask.shape
    live = mask.reshape(-1) != 0
    rowmap = live.nonzero().squeeze(-1)
    lens = mask.ne(0).sum(-1)
    woff = torch.cumsum(lens, 0) - lens
    soff = (starts + woff[:, None]).reshape(-1)
    width = (ends - starts + 1).reshape(-1)
    JR = max(0, min(int(width.max()), S))
    return rowmap, woff, soff, width, int(rowmap.numel()), JR


def index_ref(mask, starts, ends):
    """The whole index block: rowmap[B S] | fidx[B S] | woff[B] | soff[B M] | width[B M] | meta[2] as int32, and the bool mask of
    the entries it specifies (rowmap[T:] is not)."""
    B, S = mask.shape
    rowmap, woff, soff, width, T, JR = span_geometry(mask, starts, ends)
    live = mask.reshape(-1) != 0
    fidx = torch.where(live, torch.cumsum(live.long(), 0) - 1, torch.full((B * S,), -1))
    rm = torch.zeros(B * S, dtype=torch.int64)
    rm[:T] = rowmap
    block = torch.cat([rm, fidx, woff, soff, width, torch.tensor([T, JR])]).to(torch.int32)
    spec = torch.ones(block.numel(), dtype=torch.bool)
    spec[T:B * S] = False
    return block, spec


# ---------------------------------------------------------------------------------------------------------------------
# span pooling
# ---------------------------------------------------------------------------------------------------------------------
def _pc(cid, B, S, M, H, mask="ragged", spans="plain", score="plain"):
    return dict(id=cid, B=B, S=S, M=M, H=H, mask=mask, spans=spans, score=score)


POOL_H = {4: "one-lane", 252: "last-lane-of-chunk-masked", 260: "second-chunk-one-lane", 1024: "all-four-chunks-full"}
POOL_SCORES = ["plain", "ascending", "descending", "onehot50", "addmask2e4"]
POOL_CASES = [_pc("B2-S6-M3-H%d-%s" % (H, why), 2, 6, 3, H) for H, why in POOL_H.items()] + [
    _pc("B1-S5-M1-H8-NS1-three-idle-waves", 1, 5, 1, 8),
    _pc("B1-S5-M3-H8-NS3", 1, 5, 3, 8),
    _pc("B1-S5-M5-H8-NS5-second-block-one-wave", 1, 5, 5, 8),
    _pc("B1-S6-M130-H4-token-read-by-130-spans-three-ballot-rounds-masked-and-unread-rows", 1, 6, 130, 4, mask="holes",
        spans="cover-one-token"),
    _pc("B2-S6-M3-H8-clipped-positions-pile-onto-the-last-token", 2, 6, 3, 8, spans="pile-on-last"),
    _pc("B3-S7-M3-H8-masked-sentence-between-live-ones", 3, 7, 3, 8, mask="middle-empty"),
    _pc("B2-S6-M3-H8-span-wider-than-S-truncated", 2, 6, 3, 8, spans="wider-than-S"),
] + [_pc("B2-S6-M3-H%d-score-%s" % (H, k), 2, 6, 3, H, score=k, spans="pile-on-last") for k in POOL_SCORES[1:] for H in (8, 260)]
POOL_ZERO_CASES = [_pc("B2-S5-M2-H8-T0-all-masked", 2, 5, 2, 8, mask="none"),
                   _pc("B2-S6-M3-H8-JR0-all-widths-nonpositive", 2, 6, 3, 8, spans="empty")]
POOL_REJECTED_H = [0, 6, 1028]


def pool_inputs(c):
    """-> seq [B, S, H], mask u8, starts, ends, wu [1, H], bu [1], gw [B * M, H] (the upstream gradient of pooled)"""
    B, S, M, H = c["B"], c["S"], c["M"], c["H"]
    g = gen(1000 * B + 100 * S + M + H)
    mask = span_mask(B, S, c["mask"], g)
    if c["spans"] == "cover-one-token":
        mask = torch.ones(B, S, dtype=torch.uint8)
        mask[0, 3] = 0
    starts, ends = span_bounds(mask, M, c["spans"], g)
    seq = torch.randn(B, S, H, generator=g)
    wu, bu = torch.randn(1, H, generator=g) * 0.2, torch.randn(1, generator=g)
    gw = torch.randn(B * M, H, generator=g)
    kind = c["score"]
    unit = wu / wu.norm()
    if kind in ("ascending", "descending"):  # the score moves by 1.5 per token: the running maximum changes on every step
        step = 1.5 if kind == "ascending" else -1.5
        seq = seq - (seq * unit.view(1, 1, H)).sum(-1, keepdim=True) * unit.view(1, 1, H)  # (the noise along w taken out)
        seq = seq + step * torch.arange(B * S, dtype=torch.float32).view(B, S, 1) * (unit / wu.norm()).view(1, 1, H)
    elif kind == "onehot50":    # scores of standard deviation 50
        wu = unit * 50.0
    elif kind == "addmask2e4":  # scores of standard deviation 2e4: a position behind the span, at -10000, can still lead
        wu = unit * 2e4
    else:
        assert kind == "plain", kind
    return seq, mask, starts, ends, wu, bu, gw


def _pool_parts(seq, mask, starts, ends, wu, bu, dtype):
    """the reference's own lines -> emb [NS, JR, H], span mask, scores, leaves"""
    B, S, H = seq.shape
    ends = torch.minimum(ends, starts + S - 1)  # the contract of mtvaf_span_index: JR <= S truncates a wider span
    s, w, b = (t.to(dtype).requires_grad_(True) for t in (seq, wu, bu))
    emb, sm = O.span_representation(starts, ends, s, mask.long())
    score = F.linear(emb, w, b).squeeze(-1)
    return emb, sm, score, (s, w, b)


def pool_ref(seq, mask, starts, ends, wu, bu, gw, dtype=torch.float64):
    """O.span_representation + linear + O.self_att_representation, autograd for the gradients of sum(pooled * gw)
    -> pooled [B M, H], dseq [B S, H], dw [H], db [1].  T = 0 or JR = 0: all zeros (the reference cannot run there).
    dtype float32: the same lines as a plain fp32 restatement."""
    B, S, H = seq.shape
    NS = starts.numel()
    _, _, _, _, T, JR = span_geometry(mask, starts, ends)
    if T == 0 or JR == 0:
        return tuple(torch.zeros(n, dtype=dtype) for n in ((NS, H), (B * S, H), (H,), (1,)))
    emb, sm, score, (s, w, b) = _pool_parts(seq, mask, starts, ends, wu, bu, dtype)
    pooled = O.self_att_representation(emb, score, sm)
    (pooled * gw.to(dtype)).sum().backward()
    return pooled.detach(), s.grad.reshape(B * S, H), w.grad.reshape(H), b.grad.reshape(1)


def pool_terms(seq, mask, starts, ends, wu, bu, gw, cond):
    """the derived terms (float64; see the top of the file) -> dict pooled, dseq, dw, db.  db always; the others only for
    a case of POOL_COND_KINDS (cond True), None otherwise."""
    B, S, H = seq.shape
    rowmap, _, soff, _, T, JR = span_geometry(mask, starts, torch.minimum(ends, starts + S - 1))
    with torch.no_grad():
        emb, sm, score, (_, w, b) = _pool_parts(seq, mask, starts, ends, wu, bu, torch.float64)
        p = torch.softmax(score + (1.0 - sm.double()) * MASKED, -1)            # [NS, JR]
        o = (p[..., None] * emb).sum(1)
        g = gw.double()
        absdot = (emb.abs() * g[:, None, :].abs()).sum(-1) + (o.abs() * g.abs()).sum(-1)[:, None]
        dot_err = DOT_K * U32 * p * absdot                                      # |d ds_nr| from the two dot products
        out = {"pooled": None, "dseq": None, "dw": None, "db": dot_err.sum().reshape(1)}
        if not cond:
            return out
        delta = DOT_K * U32 * ((emb.abs() * w.abs().view(1, 1, H)).sum(-1) + b.abs() + (1.0 - sm.double()) * -MASKED).amax(1)
        dev = emb - o[:, None, :]
        gd = (dev * g[:, None, :]).sum(-1).abs()
        dds = 2 * delta[:, None] * p * (gd + (p * gd).sum(1, keepdim=True)) + dot_err  # |d ds_nr|
        out["pooled"] = 2 * delta[:, None] * (p[..., None] * dev.abs()).sum(1)
        out["dw"] = (dds[..., None] * emb.abs()).sum((0, 1))
        out["db"] = dds.sum().reshape(1)
        rows = rowmap[(soff[:, None] + torch.arange(JR)[None, :]).clamp(0, T - 1)]  # [NS, JR] -> b * S + s
        per = 2 * (delta[:, None] * p)[..., None] * g[:, None, :].abs() + dds[..., None] * w.abs().view(1, 1, H)
        out["dseq"] = torch.zeros(B * S, H, dtype=torch.float64).index_add_(0, rows.reshape(-1), per.reshape(-1, H))
    return out


def rows_read(mask, starts, ends):
    """bool [B S]: the token rows some span position reads"""
    B, S = mask.shape
    rowmap, _, soff, _, T, JR = span_geometry(mask, starts, ends)
    read = torch.zeros(B * S, dtype=torch.bool)
    if T and JR:
        read[rowmap[(soff[:, None] + torch.arange(JR)[None, :]).clamp(0, T - 1)].reshape(-1)] = True
    return read


# ---------------------------------------------------------------------------------------------------------------------
# distant cross entropy
# ---------------------------------------------------------------------------------------------------------------------
DCE_SHAPES = {(1, 1): "one-position", (2, 63): "last-lane-idle", (2, 64): "one-full-trip", (2, 65): "second-trip-one-lane",
              (65, 5): "mean-loop-second-trip", (3, 130): "third-trip"}
DCE_LOGITS = ["plain", "offset+1e3", "offset-1e3", "offset+1e4", "offset-1e4", "spread80", "minus1e4-where-pos0"]
DCE_OFFSET_KINDS = DCE_LOGITS[1:5]
DCE_POS = ["one-hot", "all-ones", "fractional"]  # row r takes DCE_POS[r % 3]
DCE_PRIOR = 2.5  # what `loss` holds before an accumulating call


def _dc(B, S, why, ld=2, ldd=2, scale=0.5, gout=1.7, acc=0, logits="plain", empty_row=None):
    cid = "B%d-S%d-%s-ld%d-ldd%d-%s%s" % (B, S, why, ld, ldd, logits, "-accumulate" if acc else "-over-nan")
    return dict(id=cid, B=B, S=S, ld=ld, ldd=ldd, scale=scale, gout=gout, acc=acc, logits=logits, empty_row=empty_row)


DCE_CASES = [_dc(B, S, why, acc=i % 2) for i, ((B, S), why) in enumerate(DCE_SHAPES.items())] + [
    _dc(2, 65, "strides", ld=ld, ldd=ldd, scale=1.0 + 0.25 * ld, gout=0.7, acc=ld % 2) for ld in (1, 2, 5)
    for ldd in sorted({ld, 3})] + [
    _dc(B, S, "logits", logits=k, scale=0.5, gout=1.7, acc=i % 2) for i, k in enumerate(DCE_LOGITS[1:])
    for (B, S) in ((2, 65), (3, 130))]
DCE_EMPTY_ROW_CASE = _dc(3, 5, "row-without-a-position", empty_row=1)


def dce_inputs(c):
    """-> z [B, S] and pos [B, S] fp32"""
    B, S, kind = c["B"], c["S"], c["logits"]
    g = gen(31 * B + S + len(kind))
    z = torch.randn(B, S, generator=g) * 3
    pos = torch.zeros(B, S)
    for r in range(B):
        pk = DCE_POS[r % 3]
        if pk == "one-hot":
            pos[r, (5 * r + S // 2) % S] = 1.0
        elif pk == "all-ones":
            pos[r] = 1.0
        else:
            pos[r, ::2] = 0.25
            pos[r, (r + 1) % S] = 3.0
    if kind.startswith("offset"):
        z = z + float(kind[len("offset"):])
    elif kind == "spread80":
        z = z * (80.0 / 3)
    elif kind == "minus1e4-where-pos0":
        z[pos == 0] = MASKED
    if c["empty_row"] is not None:
        pos[c["empty_row"]] = 0.0
    return z, pos


def dce_ref(z, pos, scale, gout, dtype=torch.float64):
    """-> scale * O.distant_cross_entropy, d logits of gout * that.  dtype float32: torch's log_softmax subtracts the row
    maximum first -- the shift-safe fp32 form"""
    zz = z.to(dtype).requires_grad_(True)
    loss = O.distant_cross_entropy(zz, pos.to(dtype)) * scale
    (loss * gout).backward()
    return loss.detach(), zz.grad


def dce_shift_safe_f32(z, pos, scale, gout):
    """the kernels' lines in fp32, every operation rounded: num = sum pos (z - m), value = (num - den log e) / den,
    softmax = exp((z - m) - log e)"""
    B = z.shape[0]
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    d = z - z.amax(-1, keepdim=True)
    loge = d.exp().sum(-1).log()
    den = pos.sum(-1)
    val = ((pos * d).sum(-1) - den * loge) / den
    loss = -(f(scale) * val.sum()) / B
    gg = (-(f(gout)) * f(scale) / B / den)[:, None]
    return loss, gg * (pos - (d - loge[:, None]).exp() * den[:, None])


def dce_cancelling_f32(z, pos, scale, gout):
    """the formula the kernels had: num = sum pos z, lse = m + log e kept as one float, softmax = exp(z - lse)"""
    B = z.shape[0]
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    m = z.amax(-1)
    lse = m + (z - m[:, None]).exp().sum(-1).log()
    den = pos.sum(-1)
    val = ((pos * z).sum(-1) - den * lse) / den
    loss = -(f(scale) * val.sum()) / B
    gg = (-(f(gout)) * f(scale) / B / den)[:, None]
    return loss, gg * (pos - (z - lse[:, None]).exp() * den[:, None])


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
CE_LOGITS = ["plain", "offset+1e3", "offset-1e3", "offset+1e4", "offset-1e4", "one-class-ahead-by-100"]
CE_OFFSET_KINDS = CE_LOGITS[1:5]
CE_GOUT = 0.3


def _cc(N, C, why, ignore="none", logits="plain"):
    return dict(id="N%d-C%d-%s-%s-ignore-%s" % (N, C, why, logits, ignore), N=N, C=C, ignore=ignore, logits=logits)


CE_CASES = [_cc(5, C, why) for C, why in ((1, "one-class"), (2, "two-lanes"), (63, "last-lane-idle"), (64, "full-wave-label-63"))] + [
    _cc(N, 4, why, ignore="every-third") for N, why in ((1, "one-row"), (255, "backward-block-less-one"), (256, "backward-block"),
                                                         (257, "second-backward-block"), (640, "three-backward-blocks"))] + [
    _cc(N, C, "logits", ignore="every-third", logits=k) for k in CE_LOGITS[1:] for (N, C) in ((33, 4), (5, 64))]
CE_ALL_IGNORED_CASE = _cc(5, 4, "no-row-counted", ignore="all")
CE_REJECTED_C = [0, 65]


def ce_inputs(c):
    """-> z [N, C] fp32, labels int64 [N]: rows 0 and 1 (where they exist and count) carry the labels 0 and C - 1"""
    N, C, kind = c["N"], c["C"], c["logits"]
    g = gen(17 * N + C + len(kind))
    z = torch.randn(N, C, generator=g) * 2
    lab = torch.randint(0, C, (N,), generator=g)
    lab[0] = C - 1
    if N > 1:
        lab[1] = 0
    if kind.startswith("offset"):
        z = z + float(kind[len("offset"):])
    elif kind == "one-class-ahead-by-100":  # the leading class is the label on the even rows
        lead = torch.randint(0, C, (N,), generator=g)
        z[torch.arange(N), lead] += 100.0
        lab[::2] = lead[::2]
    if c["ignore"] == "every-third":
        lab[2::3] = -100
    elif c["ignore"] == "all":
        lab[:] = -100
    return z, lab


def ce_ref(z, lab, gout=CE_GOUT, dtype=torch.float64):
    """-> F.cross_entropy (mean over the counted rows), d logits of gout * loss, sum of the row losses, count"""
    zz = z.to(dtype).requires_grad_(True)
    loss = F.cross_entropy(zz, lab)
    (loss * gout).backward()
    tot = F.cross_entropy(zz.detach(), lab, reduction="sum")
    return loss.detach(), zz.grad, tot, int((lab != -100).sum())


def ce_shift_safe_f32(z, lab):
    """the kernel's lines in fp32: rows in order, tot += (m - z_label) + log sum exp(z - m) -> loss, tot"""
    tot, cnt = torch.zeros((), dtype=torch.float32), 0
    for n in range(z.shape[0]):
        if int(lab[n]) == -100:
            continue
        m = z[n].max()
        tot = tot + ((m - z[n, lab[n]]) + (z[n] - m).exp().sum().log())
        cnt += 1
    return tot / cnt, tot


def ce_cancelling_f32(z, lab):
    """the formula the kernel had: tot += m + log sum exp(z - m) - z_label"""
    tot, cnt = torch.zeros((), dtype=torch.float32), 0
    for n in range(z.shape[0]):
        if int(lab[n]) == -100:
            continue
        m = z[n].max()
        tot = tot + (m + (z[n] - m).exp().sum().log() - z[n, lab[n]])
        cnt += 1
    return tot / cnt, tot


# ---------------------------------------------------------------------------------------------------------------------
# mask_mul
# ---------------------------------------------------------------------------------------------------------------------
MASK_MUL_GRID4 = 4096 * 256  # float4s of one trip of the capped grid
MASK_MUL_SHAPES = {(2, 1, 4): "one-float4-per-row", (5, 33, 768): "odd-rows", (3, 342, 4096): "second-stride-trip"}
MASK_MUL_KEEPS = ["row", "col", "both"]
MASK_MUL_P = 0.3
MASK_MUL_REJECTED_H = 6


def mask_mul_id(shape, which):
    B, S, H = shape
    return "B%d-S%d-H%d-%s-%s-keep" % (B, S, H, MASK_MUL_SHAPES[shape], which)


def mask_mul_inputs(B, S, H, which):
    """-> x [B, S, H], row_keep [B * S] or None, col_keep [B, H] or None with values 0, 1 and float32(1 / (1 - p))"""
    g = gen(B + 3 * S + H)
    x = torch.randn(B, S, H, generator=g)
    vals = torch.tensor([0.0, 1.0, 1.0 / (1.0 - MASK_MUL_P)], dtype=torch.float32)
    row = vals[torch.randint(0, 3, (B * S,), generator=g)] if which in ("row", "both") else None
    col = vals[torch.randint(0, 3, (B, H), generator=g)] if which in ("col", "both") else None
    return x, row, col


def mask_mul_ref(x, row, col):
    """fp32 (x * row) * col in that order: two correctly rounded products, bit for bit what the kernel must return"""
    B, S, H = x.shape
    out = x.clone()
    if row is not None:
        out = out * row.view(B, S, 1)
    if col is not None:
        out = out * col.view(B, 1, H)
    return out
