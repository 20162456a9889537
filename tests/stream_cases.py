"""Case tables, input builders and plain float64 references of the streaming, packing and prompt kernels (csrc/optim.hip,
csrc/prompt.hip, the packing / reduction / dropout entries of csrc/rowops.hip, mtvaf_cast_bf16 / mtvaf_colsum_small), shared by
test_stream_cases.py (CPU: proves the references and the tolerances) and test_stream_kernels_gpu.py (the kernels).  Nothing
here imports mtvaf_amd: the references are numpy / torch on the host.

Every case is the smallest shape at which its kernel can still go wrong; the ids name the branch a case is there for."""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 7.25  # guard value around every view (exact in fp32 and bf16)
GUARD = 8        # guard elements on both sides of a view


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp32(x):
    """float64 tensor: the spacing of fp32 at |x| (the smallest denormal at 0)"""
    a = np.abs(np.asarray(torch.as_tensor(x).double().numpy())).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def close_excess(got, ref, rtol, atol=None):
    """The `close` of test_ops_gpu.py as a number: max over the elements of err / allowed (<= 1 passes, <= 0.25 is the
    four-fold headroom a fp32 restatement on the host must show)."""
    got = got.detach().double().cpu()
    ref32 = ref.detach().float().cpu().double()  # (`close` compares in fp32)
    if atol is None:
        atol = rtol * float(ref32.abs().max()) + 1e-7
    return float(((got.float().double() - ref32).abs() / (atol + rtol * ref32.abs())).max())


def norm_excess(got, ref, rtol):
    """max |got - ref| / (rtol * max |ref|): the bound of the kernels that had none before (mean_l, gate_fwd)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (rtol * float(ref.abs().max())))


# inherited bounds (test_ops_gpu.py): `close` rtol of split mean / mix forward, mix gradients, KL loss, KL gradient (rtol, atol),
# column sums; new: normwise rtol of mean_l and gate_fwd against float64 (a handful of fp32 operations per output)
RTOL_SPLIT_MEAN = RTOL_MIX_FWD = 2e-4
RTOL_MIX_GRAD = 1e-3
RTOL_KL_LOSS = 1e-5
RTOL_KL_GRAD, ATOL_KL_GRAD = 1e-4, 1e-8
RTOL_COLSUM = 5e-4
RTOL_MEAN_L = RTOL_GATE = 1e-6
# sum of a gate group: inv = fl(1 / S) and gate_k = fl(e_k * inv) with S = the fp32 sum of the four e_k (three roundings):
# |sum_k gate_k - 1| <= 5 * 2^-24 to first order; 4 * 2^-23 bounds it
GATE_SUM_TOL = 4 * 2.0 ** -23


def view_layout(sizes_shifts, align=4):
    """Offsets of views inside ONE flat allocation: every view starts `align` elements aligned (16 bytes for fp32) plus its
    shift, with at least GUARD guard elements on both sides.  -> (offsets, total length)"""
    offs, cur = [], 0
    for n, shift in sizes_shifts:
        o = (cur + GUARD + align - 1) // align * align + shift
        offs.append(o)
        cur = o + n
    return offs, (cur + GUARD + align - 1) // align * align


def guard_mask(total, offs, sizes):
    """bool [total]: True outside every view"""
    g = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        g[o:o + n] = False
    return g


# ---------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
# name -> (lr, weight decay, first step, zero state)
ADAM_HYPER = {"step1-zero-state": (1e-3, 1e-2, 1, True), "step2-lr5e-2-wd0": (5e-2, 0.0, 2, False),
              "step100000": (1e-3, 1e-2, 100000, False)}
ADAM_FULL_GRID = 2048 * 256 * 4  # elements of one trip of the full-width grid (stream_grid: 2048 blocks x 256 lanes x 4)
# (id, n, shifts of the p / g / m / v bases in floats, shadow: None / 0 / 1 (offset in bf16 elements), max_blocks, hyper, grad_scale)
ADAM_CASES = [
    ("n1", 1, (0, 0, 0, 0), None, 0, "step1-zero-state", 1.0),
    ("n3-tail-only", 3, (0, 0, 0, 0), 0, 0, "step2-lr5e-2-wd0", 1.0),
    ("n4-one-vector", 4, (0, 0, 0, 0), None, 0, "step100000", 1.0),
    ("n5-vector-path-with-tail", 5, (0, 0, 0, 0), 0, 0, "step1-zero-state", 1.0 / 1024),
    ("n1023-vector-path-with-tail", 1023, (0, 0, 0, 0), None, 0, "step2-lr5e-2-wd0", 1.0 / 1024),
    ("n4097-vector-path-with-tail", 4097, (0, 0, 0, 0), None, 0, "step1-zero-state", 1.0),
    ("n4097-max-blocks3-stride-trip", 4097, (0, 0, 0, 0), 0, 3, "step100000", 1.0 / 1024),
    ("n5-p-offset-scalar-path-of-adamw_span", 5, (1, 0, 0, 0), None, 0, "step2-lr5e-2-wd0", 1.0),
    ("n4097-p-offset-scalar-path-of-adamw_span", 4097, (1, 0, 0, 0), None, 0, "step1-zero-state", 1.0),
    ("n1023-g-offset-scalar-path-of-adamw_span-max-blocks3", 1023, (0, 1, 0, 0), 0, 3, "step100000", 1.0),
    ("n4097-shadow-aligned", 4097, (0, 0, 0, 0), 0, 0, "step2-lr5e-2-wd0", 1.0),
    ("n4097-unaligned-shadow", 4097, (0, 0, 0, 0), 1, 0, "step1-zero-state", 1.0),
    ("n1023-p-offset-shadow-aligned", 1023, (1, 0, 0, 0), 0, 0, "step100000", 1.0 / 1024),
    ("n%d-second-stride-trip-of-the-full-grid" % (ADAM_FULL_GRID + 13), ADAM_FULL_GRID + 13, (0, 0, 0, 0), 0, 0,
     "step1-zero-state", 1.0),
]


def adam_inputs(n, zero_state, seed):
    """-> p, m, v and the gradients of two consecutive steps (fp32).  Planted at the head (and, from n = 8, mirrored at the
    tail, so that the vector body and the scalar tail both see them): g == 0; m == v == 0; |g| = 1e-20 on a zero state (its
    square underflows: v is a denormal); |p| = 1e4."""
    g = gen(seed)
    p = torch.randn(n, generator=g)
    g1, g2 = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    if zero_state:
        m.zero_(), v.zero_()
    spots = [0, 1, 2, 3] + ([n - 1, n - 2, n - 3, n - 4] if n >= 8 else [])
    for k, i in enumerate(spots):
        if i >= n:
            continue
        kind = k % 4
        if kind == 0:
            g1[i] = 0.0
            g2[i] = 0.0
        elif kind == 1:
            m[i] = 0.0
            v[i] = 0.0
        elif kind == 2:
            m[i] = 0.0
            v[i] = 0.0
            g1[i] = 1e-20
            g2[i] = -1e-20
        else:
            p[i] = -1e4 if k > 3 else 1e4
    return p, m, v, (g1, g2)


def adamw_ref(p, g, m, v, lr, wd, step, grad_scale=1.0):
    """One step of decoupled-weight-decay Adam as torch.optim.AdamW states it, float64 throughout, python-double
    hyper-parameters.  fp32 (or float64) inputs -> float64 p, m, v."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * grad_scale
    p = p * (1.0 - lr * wd)
    m = BETA1 * m + (1.0 - BETA1) * g
    v = BETA2 * v + (1.0 - BETA2) * g * g
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + EPS
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adamw_f32(p, g, m, v, lr, wd, step, grad_scale=1.0):
    """The update of adamw1 (csrc/optim.hip) in fp32 on the host, every operation rounded on its own, no fused multiply-add (the
    device's own sequence, with its fmas, is adamw_pinned below); the hyper-parameters rounded as make_hyper and the wrapper round
    them."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    bc1, bc2s = f(1.0 - BETA1 ** step), f((1.0 - BETA2 ** step) ** 0.5)
    lr_, wd_, gs = f(lr), f(wd), f(grad_scale)
    omb1, omb2, b2, eps = f(1.0 - BETA1), f(1.0 - BETA2), f(BETA2), f(EPS)
    g = g * gs
    p = p - (lr_ * wd_) * p
    m = m + omb1 * (g - m)
    v = b2 * v + (omb2 * g) * g
    denom = v.sqrt() / bc2s + eps
    p = p - (lr_ / bc1) * (m / denom)
    return p, m, v


def _round32(x):
    """Fraction -> the nearest float32 (ties to even; gradual underflow), as a Fraction."""
    if x == 0:
        return x
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if Fraction(n, d) < Fraction(2) ** e:
        e -= 1  # 2^e <= |x| < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    return round(x / quantum) * quantum  # (round() of a Fraction: half to even)


PINNED_N = 64  # elements of the bit-for-bit device tests: one block, 16 float4s; the exact arithmetic below takes ~10 ms per element


def pinned_inputs(seed, n=PINNED_N):
    """adam_inputs without the planted elements (no denormal, no 1e-20 gradient: flushing is not part of the pinned contract)."""
    g = gen(seed)
    p = torch.randn(n, generator=g)
    g1, g2 = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    return p, m, v, (g1, g2)


def adamw_pinned(p, g, m, v, lr, wd, step, grad_scale=1.0):
    """The rounding sequence adamw1 (csrc/optim.hip) pins, in exact rational arithmetic with ONE correctly rounded conversion to
    float32 per line; hyper-parameters rounded as make_hyper and the wrapper round them.  fp32 in, fp32 out -- the device's bits.
        gs  = g * s
        d   = fma(g, s, -m)                     (not gs - m)
        m   = fma(omb1, d, m)
        v   = fma(beta2, v, gs * (omb2 * gs))
        p1  = fma(-(lr * wd), p, p)
        den = sqrt(v) / bc2_sqrt + eps
        p   = fma(-(lr / bc1), m / den, p1)"""
    f = lambda x: Fraction(float(torch.tensor(x, dtype=torch.float32)))
    r = _round32
    s, lr_, wd_, eps = f(grad_scale), f(lr), f(wd), f(EPS)
    omb1, omb2, b2 = f(1.0 - BETA1), f(1.0 - BETA2), f(BETA2)
    bc1, bc2s = f(1.0 - BETA1 ** step), f((1.0 - BETA2 ** step) ** 0.5)
    lrwd, lrbc = r(lr_ * wd_), r(lr_ / bc1)
    out = [], [], []
    for pi, gi, mi, vi in zip(*(t.double().tolist() for t in (p, g, m, v))):
        pi, gi, mi, vi = Fraction(pi), Fraction(gi), Fraction(mi), Fraction(vi)
        gs = r(gi * s)
        d = r(gi * s - mi)
        mi = r(omb1 * d + mi)
        vi = r(b2 * vi + r(gs * r(omb2 * gs)))
        p1 = r(-lrwd * pi + pi)
        root = Fraction(float(torch.tensor(math.sqrt(float(vi)), dtype=torch.float32)))  # (float64 sqrt of a float32, rounded: exact)
        den = r(r(root / bc2s) + eps)
        pi = r(-lrbc * r(mi / den) + p1)
        for o, x in zip(out, (pi, mi, vi)):
            o.append(float(x))
    return tuple(torch.tensor(o, dtype=torch.float64).float() for o in out)  # (every value is a float32: the conversion is exact)


def adam_errors(got, ref, p_old, m_old, g, lr, grad_scale=1.0):
    """Errors of one step (got: fp32 p, m, v; ref: float64) -> dict of maxima:
      p_lr   |dp| / (ulp(|p|) + lr)              the unit the optimizer tests are stated in;
      p_ulp  |dp| / (ulp(|p|) + ulp(|p - p_old|)) derived: the result is rounded at ulp(p) (twice: decay, update), the update is a
             product of a few correctly rounded operations, so it is off by a few ulp OF ITSELF -- a wrong update of the order of
             lr passes p_lr and fails this one;
      m      in ulp of the largest of |m_old|, |(1 - beta1) g| and |m|: the ulp of a sum is that of its largest term (0.9 m_old
             and 0.1 g cancel in some of two million elements, and the ulp of what is left says nothing about the addition);
      v      in ulp of the reference value (a sum of non-negative terms)."""
    (gp, gm, gv), (rp, rm, rv) = got, ref
    dp = (gp.double() - rp).abs()
    m_top = torch.maximum(torch.maximum(m_old.double().abs(), (1.0 - BETA1) * grad_scale * g.double().abs()), rm.abs())
    return {"p_lr": float((dp / (ulp32(rp) + lr)).max()),
            "p_ulp": float((dp / (ulp32(rp) + ulp32(rp - p_old.double()))).max()),
            "m": float(((gm.double() - rm).abs() / ulp32(m_top)).max()),
            "v": float(((gv.double() - rv).abs() / ulp32(rv)).max())}


# Largest error of adamw_f32 against adamw_ref over ADAM_CASES, ADAM_MULTI_CASES and the planes case, both steps, every step taken
# from the fp32 state actually fed to it (test_stream_cases.py::test_adamw_fp32_restatement_error_is_the_recorded_one recomputes
# them).  Measured at commit c3aefca: p_lr 0.4403, p_ulp 5.2146, m 2.4500, v 2.5712.
# The device may contract multiply-adds (fewer roundings) and orders nothing else differently: it is allowed ADAM_DEVICE_FACTOR
# times these.
ADAM_F32_ERR = {"p_lr": 0.45, "p_ulp": 5.3, "m": 2.5, "v": 2.6}
ADAM_DEVICE_FACTOR = 4.0

# adamw_multi: count members, sizes cycling through ADAM_MULTI_SIZES, every third member an unaligned view (all four bases
# offset by one float); the count-49 case carries one member one stride trip past the per-tensor block cap (1024 blocks)
ADAM_MULTI_SIZES = [1, 2, 5, 64, 1000, 4099]
ADAM_MULTI_BIG = 1024 * 256 * 4 + 7
ADAM_MULTI_HYPER = (1e-3, 1e-2, 3)  # lr, wd, step
# (id, count, index of the big member or None)
ADAM_MULTI_CASES = [("count1", 1, None), ("count48-one-full-launch", 48, None),
                    ("count49-second-launch-and-a-member-past-the-block-cap", 49, 10),
                    ("count97-three-launches", 97, None)]


def adam_multi_members(count, big):
    """-> [(n, shift)]"""
    return [(ADAM_MULTI_BIG if i == big else ADAM_MULTI_SIZES[i % len(ADAM_MULTI_SIZES)], 1 if i % 3 == 2 else 0)
            for i in range(count)]


# adamw_planes: matrices (rows, cols) and the gaps behind them in one flat buffer (n % 4 == 0)
PLANES_SHAPES = [(96, 64), (64, 64), (128, 64), (64, 128)]
PLANES_GAPS = [96, 64 + 8, 128 + 4, 64]
PLANES_HYPER = (1e-3, 1e-2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# bf16 wire format
# ---------------------------------------------------------------------------------------------------------------------
STREAM_GRID8 = 2048 * 256  # 8-element vectors of one trip of the capped grid
# exact ties both ways (to even: down, up), signed zeros, infinities, a value above the bf16 maximum (rounds to inf), bf16
# denormals (exact, and a tie between two of them), fp32 denormals, NaN last (compared by isnan only)
PLANTED = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0, float("inf"), -float("inf"), 3.4e38, -3.4e38,
           2.0 ** -133, 3 * 2.0 ** -133, 1.5 * 2.0 ** -133, 1e-40, -1e-40, 1e-45, 2.0 ** -127, float("nan")]
# (n, extra padding behind n rounded up to 8)
PACK_CASES = [(1, 0), (7, 0), (8, 0), (9, 0), (9, 64), (100003, 0), (8 * STREAM_GRID8 + 3, 0)]
# (W, chunk, scale)
REDUCE_CASES = [(1, 8, 1.0), (2, 8, 0.5), (8, 8, 0.125), (1, 8 * 257, 1.0), (2, 8 * 257, 1.0), (2, 8 * 257, 0.5),
                (8, 8 * 257, 1.0), (8, 8 * 257, 0.125), (2, 8 * (STREAM_GRID8 + 3), 0.5)]
UNPACK_CASES = [1, 7, 8, 9, 100003]


def planted_f32(n, seed):
    x = torch.randn(n, generator=gen(seed))
    k = min(n, len(PLANTED))
    x[:k] = torch.tensor(PLANTED[:k], dtype=torch.float32)
    return x


def bf16_round_ref(x):
    """fp32 -> bf16, round to nearest, ties to even, in integer arithmetic on the bit patterns (NaN: quiet NaN)"""
    u = x.contiguous().view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)
    return torch.from_numpy(r.view(np.int16).copy()).view(torch.bfloat16)


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bf16(got, want):
    """bit-exact, NaN positions by isnan only"""
    got, want = got.cpu(), want.cpu()
    nan = want.float().isnan()
    return bool(torch.equal(got.float().isnan(), nan)) and bool(torch.equal(bits16(got)[~nan], bits16(want)[~nan]))


def reduce_inputs(W, chunk, seed):
    return torch.randn(W * chunk, generator=gen(seed)).to(torch.bfloat16)


def reduce_ref(recv, W, chunk, scale):
    """fp32 sum in rank order, one multiplication, one rounding"""
    acc = torch.zeros(chunk, dtype=torch.float32)
    for r in range(W):
        acc = acc + recv[r * chunk:(r + 1) * chunk].float()
    return bf16_round_ref(acc * torch.tensor(scale, dtype=torch.float32))


def unpack_inputs(n, seed):
    """bf16 source padded to 8 with the exactly representable planted values (no NaN)"""
    npad = (n + 7) // 8 * 8
    src = torch.randn(npad, generator=gen(seed)).to(torch.bfloat16)
    special = torch.tensor([-0.0, float("inf"), -float("inf"), 2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -127, 1 + 2.0 ** -7],
                           dtype=torch.float32).to(torch.bfloat16)
    k = min(n, len(special))
    src[:k] = special[:k]
    return src


# ---------------------------------------------------------------------------------------------------------------------
# prompt generator pieces
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_MEAN_CASES = [(1, 4), (3, 8), (48, 1536), (1400, 1536)]  # (rows, W); the last: more float4s than 2048 x 256 lanes


def split_mean_id(c):
    return "rows{}-W{}".format(*c) + ("-stride-loop" if c[0] * (c[1] // 4) > 2048 * 256 else "")


def split_mean_ref(enc, rows, W):
    return enc.double().view(rows, 4, W).mean(1)


GATE_GROUPS = [1, 255, 256, 257]
# "minus100": random logits around -100.  Random logits around -1e4 cannot be held to RTOL_GATE by ANY fp32 evaluation (0.01 * z
# rounds at ulp(100) = 7.6e-6, which the exponential turns into a relative error of 4e-6: the host restatement misses the
# four-fold headroom), so the scale of the random case is reduced and -1e4 itself is there as a constant, where the result is
# exactly 1/4
GATE_MODES = ["scale1", "scale80", "minus100", "minus1e4-constant", "all-equal"]


def gate_logits(ngroups, mode, seed=5):
    z = torch.randn(ngroups, 4, generator=gen(seed + ngroups))
    if mode == "scale80":
        z = z * 80
    elif mode == "minus100":
        z = z - 100
    elif mode == "minus1e4-constant":
        z = torch.full_like(z, -1e4)
    elif mode == "all-equal":
        z = z[:, :1].expand(-1, 4).contiguous()
    return z


def gate_ref(z):
    return torch.softmax(F.leaky_relu(z.double(), 0.01), -1)


MIX_DEPTHS = [2, 3, 4, 6, 8, 12, 24]
# (NL, NI, B, Lp, W)
MIX_CASES = [(NL, 2, 2, 2, 256) for NL in MIX_DEPTHS] + [(3, 2, 2, 2, W) for W in (8, 264, 1536, 3072)] + \
            [(3, 1, 1, 1, 256), (3, 4, 3, 4, 256)]
MIX_REJECTED = [(1, 256), (5, 256), (3, 12)]  # (NL, W): depths the dispatch does not instantiate, W % 8 != 0


def mix_id(c):
    NL, NI, B, Lp, W = c
    q = W // 4
    geo = "block%d" % q if (q <= 384 and q % 64 == 0) else (
        "256-thread-fallback-wraps-kv-boundary-in-second-trip" if W > 1024 else "256-thread-fallback")
    return "NL{}-NI{}-B{}-Lp{}-W{}-{}".format(NL, NI, B, Lp, W, geo)


def mix_inputs(NL, NI, B, Lp, W):
    """-> enc [NI,B,Lp,4W], gate logits [NI*B, NL*4] (one planted at exactly 0, where the kernel and torch both take the negative
    slope; the last row large and negative: -100 to -200, not -1000, where the fp32 rounding of 0.01 * z alone costs the gate the
    four-fold headroom of RTOL_GATE), upstream gradients of pkv [NL,2,B,NI*Lp*W/2] and of the split mean [NI*B, Lp*W]"""
    n, hid = NI * B, W // 2
    g = gen(100 * NL + W + NI)
    enc = torch.randn(NI, B, Lp, 4 * W, generator=g)
    z = torch.randn(n, NL * 4, generator=g)
    z[n - 1] = -100.0 * (1 + torch.rand(NL * 4, generator=g))
    z[0, 1] = 0.0
    gk = torch.randn(NL, 2, B, NI * Lp * hid, generator=g)
    dsm = torch.randn(n, Lp * W, generator=g)
    return enc, z, gk, dsm


def mix_ref(enc, z, gk, dsm, NL, NI, B, Lp, W, dtype=torch.float64):
    """The composition of test_prompt_mix with the projector's logits as an input: -> sm, gate, pkv, d logits, d enc of
    L = sum(pkv * gk) + sum(sm * dsm).  dtype float32: the same formula as a plain fp32 restatement."""
    n, hid = NI * B, W // 2
    e = enc.to(dtype).requires_grad_(True)
    zz = z.to(dtype).requires_grad_(True)
    sm = e.view(NI, B, Lp, 4, W).mean(3).reshape(n, Lp * W)
    gate = torch.softmax(F.leaky_relu(zz).view(n, NL, 4), -1)
    kv = torch.einsum("nik,nlkc->nilc", gate, e.view(n, Lp, 4, W))  # [n, NL, L, W]
    kv = kv.view(NI, B, NL, Lp, W).permute(2, 1, 0, 3, 4).reshape(NL, B, NI * Lp, W)
    pkv = torch.stack([kv[..., :hid].reshape(NL, B, -1), kv[..., hid:].reshape(NL, B, -1)], 1)
    ((pkv * gk.to(dtype)).sum() + (sm * dsm.to(dtype)).sum()).backward()
    return sm.detach(), gate.detach().reshape(n, NL * 4), pkv.detach(), zz.grad, e.grad


KL_SHAPES = [(1, 1), (1, 255), (2, 256), (3, 257), (5, 2089), (65, 300), (130, 7)]
KL_LOGITS = ["scale2", "scale30", "scale2-offset1e4"]
KL_TARGET_KINDS = ["softmax", "leading-zeros", "one-hot", "all-zero", "sums-to-half"]
KL_GOUT, KL_GSCALE = 0.7, 2.0


def kl_id(B, N, mode):
    return "B{}-N{}-{}".format(B, N, mode) + ("-fewer-elements-than-threads" if N < 256 else "") + \
        ("-mean-rows-loop" if B > 64 else "")


def kl_inputs(B, N, mode):
    """Row r of the target is of kind KL_TARGET_KINDS[(r + N) % 5]: every shape with five rows or more has every kind, the
    others take turns.  The one-hot row puts its mass on the row's largest logit but one: on the largest, softmax - 1 cancels
    to nothing at logit scale 30, and ANY fp32 evaluation misses rtol 1e-4 / atol 1e-8 there (scale reduced, as the tolerance
    rules ask: the cancellation is the formula's, not a kernel's)."""
    g = gen(31 * B + N)
    z = torch.randn(B, N, generator=g) * (30.0 if mode == "scale30" else 2.0)
    if mode == "scale2-offset1e4":
        z = z + 1e4
    t = torch.softmax(torch.randn(B, N, generator=g), -1)
    for r in range(B):
        kind = KL_TARGET_KINDS[(r + N) % 5]
        if kind == "leading-zeros":
            t[r, :min(10, N - 1)] = 0
        elif kind == "one-hot":
            hot = int(z[r].argsort(descending=True)[min(1, N - 1)])
            t[r] = 0
            t[r, hot] = 1
        elif kind == "all-zero":
            t[r] = 0
        elif kind == "sums-to-half":
            t[r] = t[r] * 0.5
    return z, t


def kl_ref(z, t, dtype=torch.float64):
    """-> loss, d logits of gout * gscale * loss"""
    zz = z.to(dtype).requires_grad_(True)
    loss = F.kl_div(F.log_softmax(zz, -1), t.to(dtype), reduction="batchmean")
    (loss * KL_GOUT * KL_GSCALE).backward()
    return loss.detach(), zz.grad


MEAN_L_CASES = [(1, 1, 4), (3, 4, 8), (7, 5, 12), (5, 3, 6144), (350, 4, 6144)]  # (n, L, W4)


def mean_l_id(c):
    n, L, W4 = c
    return "n{}-L{}-W{}".format(n, L, W4) + ("-stride-loop" if n * (W4 // 4) > 2048 * 256 else "")


def mean_l_inputs(n, L, W4):
    g = gen(n + L + W4)
    return torch.randn(n, L, W4, generator=g), torch.randn(n, W4, generator=g), torch.randn(n, L, W4, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
# (id, B, S, P, mask kind, masked value, prefix columns masked)
PACK_MASK_CASES = [
    ("B1-S1-all-kept", 1, 1, 0, "all", -10000.0, False),
    ("B1-S1-nothing-kept", 1, 1, 0, "none", -10000.0, False),
    ("B1-S63-ragged", 1, 63, 0, "ragged", -10000.0, False),
    ("B2-S64-P4-holes-masked-prefix-columns-ignored", 2, 64, 4, "holes", -10000.0, True),
    ("B3-S65-P36-ragged-one-sentence-all-masked", 3, 65, 36, "ragged-one-empty", -10000.0, False),
    ("B17-S100-P16-more-sentences-than-waves-holes-minus-inf", 17, 100, 16, "holes", -float("inf"), False),
    ("B40-S130-ragged-one-sentence-all-masked", 40, 130, 0, "ragged-one-empty", -10000.0, False),
    ("B300-S7-P4-holes-many-length-ties", 300, 7, 4, "holes", -10000.0, False),
]


def packing_mask(B, S, P, kind, masked, prefix_masked):
    """-> additive mask fp32 [B, P + S]"""
    g = gen(1000 * B + S)
    if kind == "all":
        keep = torch.ones(B, S, dtype=torch.bool)
    elif kind == "none":
        keep = torch.zeros(B, S, dtype=torch.bool)
    elif kind == "holes":
        keep = torch.rand(B, S, generator=g) < 0.6
    else:
        lens = torch.randint(1, S + 1, (B,), generator=g)
        keep = torch.arange(S)[None, :] < lens[:, None]
        if kind == "ragged-one-empty":
            keep[B // 2] = False
    m = torch.zeros(B, P + S)
    m[:, P:][~keep] = masked
    if prefix_masked:
        m[:, :P] = -10000.0
    return m


def packing_ref(addmask, P, S, ordered=False):
    """-> cu [B+1] (ordered: [2B+1], cu[0] = -1, the sentences by length descending, ties by index, behind the offsets), inv
    [B*S], rowmap [B*S], mv; int32 numpy.  A token is kept when its additive mask value is above -5000."""
    m = addmask.numpy()
    B = m.shape[0]
    keep = (m[:, P:] > -5000.0).reshape(-1)
    lens = keep.reshape(B, S).sum(1)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    mv = int(cu[B])
    rowmap = np.full(B * S, -1, np.int32)
    rowmap[:mv] = np.flatnonzero(keep)
    inv = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    if ordered:
        order = sorted(range(B), key=lambda b: (-int(lens[b]), b))
        cu = np.concatenate([cu, np.asarray(order, np.int32)])
        cu[0] = -1
    return cu, inv, rowmap, mv


# (bk, B, S) with B * S % bk == 0, each under every liveness pattern that fits its tile count
KTILE_SHAPES = [(32, 1, 32), (32, 4, 48), (64, 4, 48), (32, 6, 16), (32, 63, 32), (32, 64, 32), (64, 64, 32), (32, 65, 32),
                (32, 100, 64), (64, 100, 64)]
KTILE_PATTERNS = ["all-live", "dead-start-middle-end", "one-tile-live-in-its-last-row-only", "nothing-live"]
KTILE_P = 3


def ktile_id(bk, B, S, pattern):
    nt = B * S // bk
    return "bk{}-B{}-S{}-{}tiles{}-{}".format(bk, B, S, nt, "-straddling-sentences" if S % bk else "", pattern)


def ktile_mask(bk, B, S, pattern):
    """-> additive mask [B, KTILE_P + S] whose tiles of bk rows of the flat token axis are live / dead by `pattern`"""
    nt = B * S // bk
    g = gen(bk + 7 * B + S)
    keep = torch.rand(nt, bk, generator=g) < 0.3
    keep[:, 0] |= ~keep.any(1)  # a live tile has a live token
    if pattern == "dead-start-middle-end":
        keep[[0, nt // 2, nt - 1]] = False
    elif pattern == "one-tile-live-in-its-last-row-only":
        keep[:] = False
        keep[nt // 2, bk - 1] = True
    elif pattern == "nothing-live":
        keep[:] = False
    m = torch.zeros(B, KTILE_P + S)
    m[:, KTILE_P:][~keep.reshape(B, S)] = -10000.0
    return m


def ktiles_ref(addmask, P, S, bk):
    """-> (list of the live tiles in order, their count)"""
    keep = (addmask.numpy()[:, P:] > -5000.0).reshape(-1, bk)
    live = np.flatnonzero(keep.any(1)).astype(np.int32)
    return live, len(live)


GATHER_CASES = [(1, 4), (128, 8), (300, 768), (5000, 1028)]  # (rows_dst, H); the last: more float4s than 4096 x 256 lanes
GATHER_MAPS = ["random-with-minus1-and-duplicates", "reversed-permutation"]


def gather_inputs(rows, H, kind):
    """-> src [rows + 3, H], map int32 [rows]"""
    g = gen(rows + H)
    src = torch.randn(rows + 3, H, generator=g)
    if kind == "reversed-permutation":
        mp = torch.arange(rows - 1, -1, -1, dtype=torch.int32)
    else:
        mp = torch.randint(0, rows + 3, (rows,), generator=g).to(torch.int32)
        mp[::3] = -1
        if rows > 4:
            mp[4] = mp[1]
    return src, mp


def gather_ref(src, mp):
    out = src[mp.long().clamp(min=0)].clone()
    out[mp < 0] = 0
    return out


ZERO_SIZES = [1, 3, 4, 5, 4096 * 256 * 4 + 5]  # the last: one stride trip past the 4096-block cap


# ---------------------------------------------------------------------------------------------------------------------
# reductions, casts, dropout
# ---------------------------------------------------------------------------------------------------------------------
COLSUM_ROWS = [1, 511, 512, 513, 4097]  # <= 512 rows: colsum_direct_kernel, above: the two-stage kernels
COLSUM_COLS = [1, 31, 32, 33, 65, 768]
COLSUM_STRIDED = [(511, 33, 40), (4097, 33, 40)]  # (rows, cols, ld)
COLSUM_SMALL_ROWS, COLSUM_SMALL_COLS = [1, 2, 255, 256], [1, 33, 768]


def colsum_id(rows):
    return "rows%d-%s" % (rows, "direct-kernel" if rows <= 512 else "two-stage-kernels")


def colsum_inputs(rows, cols, ld=None):
    """-> x [rows, ld or cols] (the view [:, :cols] is summed), the prior content of `out` for the accumulating form"""
    g = gen(rows * 1000 + cols)
    return torch.randn(rows, ld or cols, generator=g), torch.randn(cols, generator=g)


CAST_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (100, 768)]
CAST_OUTPUTS = ["out", "out_t", "both"]
CAST_PADS = (3, 5, 7)  # extra leading dimension of x / out / out_t in the strided form


def cast_inputs(R, C):
    return planted_f32(R * C, seed=R * 100 + C).view(R, C)


DROPOUT_N = 1 << 21
DROPOUT_PS = [0.1, 0.5, 0.9]
DROPOUT_STRIDE_N = 4 * (2048 * 256 + 3)


def dropout_scale(p):
    """float32(1 / (1 - p)) from the double p, as torch scales the kept elements"""
    return np.float32(1.0 / (1.0 - float(p)))


def keep_fraction_bound(p, count):
    """five standard deviations of the mean of `count` independent Bernoulli(1 - p) draws"""
    return 5.0 * math.sqrt(p * (1.0 - p) / count)
