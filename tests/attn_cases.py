"""Cases, float64 reference and dropout-mask replica shared by the prefix-attention contract tests (test_attn_cases.py on the
CPU, test_attention_contract_gpu.py on the GPU).  No GPU import here.

Layouts are the C-ABI's: qkv [B*S, 3H] = Q | K | V with head h in columns h*64 .. h*64+63 of each third, pk / pv [B, NH*P*64]
= [B, NH, P, 64], addmask [B, P+S] additive (0 / -10000), ctx / dctx [B*S, H], lse / delta [B, NH, S], dpk / dpv as pk / pv.
The CPU file asserts that every case has the property its name states and that the reference's autograd gradients agree with
the closed-form softmax backward."""
from dataclasses import dataclass

import numpy as np
import torch

D = 64
KT = 64  # keys per tile of the kernels
SCALE = 0.125


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    S: int
    P: int
    NH: int
    lengths: tuple                      # unmasked text tokens per sentence (a prefix of the text axis, before the holes)
    holes: tuple = ()                   # (sentence, text position) masked inside the unmasked run
    masked_prefix: tuple = ()           # (sentence, prefix slot) masked
    qk_scale: float = 1.0               # Q and K are unit normals times this
    ramp: tuple = ()                    # (sentence, factor at key 0, factor at key T-1): K rows scaled along the key index
    seed: int = 0

    @property
    def T(self):
        return self.P + self.S

    @property
    def H(self):
        return self.NH * D

    @property
    def exempt(self):
        """Sentences with EVERY key masked (so P = 0): fp32 cannot follow float64 there.  Derived from the mask, never declared."""
        return tuple(b for b in range(self.B) if not bool(mask_of(self)[b].any()))

    @property
    def suffix_masked(self):
        """Whether the packed layout can run it: every mask is a trailing cut and no sentence is empty."""
        return not self.holes and not self.masked_prefix and not self.exempt and min(self.lengths) >= 1

    def __str__(self):
        return self.name


CASES = [
    # (the lengths of the packed cases are deliberately not in descending order: their ordered launch list is no identity)
    # one partial query tile, no prefix; NH*B = 6: the XCD regrouping is the identity
    Case("s16_p0", B=3, S=16, P=0, NH=2, lengths=(16, 1, 9), seed=1),
    # T = 106: the second key tile has 3 live 16-key blocks; a hole at text position 3, another at text position 0
    Case("t106_two_holes", B=3, S=70, P=36, NH=2, lengths=(70, 1, 37), holes=((0, 3), (2, 0)), seed=2),
    # T = 128 exactly on a key tile; effective T = 127, 128 and 65 (one past a tile)
    Case("t128_on_tile", B=3, S=64, P=64, NH=2, lengths=(63, 64, 1), seed=3),
    # odd prefix: the prefix / text boundary falls inside a 4-key register group; T = 128; the second query tile holds ONE query;
    # the short sentence ends exactly on the first key tile (T = 64).  NH*B = 8: the XCD regrouping is live
    Case("odd_prefix_p63", B=2, S=65, P=63, NH=4, lengths=(1, 65), seed=4),
    # three query tiles with a 2-query remainder, a one-slot prefix.  NH*B = 8
    Case("three_qtiles_p1", B=2, S=130, P=1, NH=4, lengths=(65, 130), seed=5),
    # lengths on 16-block edges; with P = 16 the key counts are 31, 32, 33, 64, 65
    Case("block_edges", B=5, S=49, P=16, NH=1, lengths=(15, 16, 17, 48, 49), seed=6),
    # prefix slots 0..63 masked: the first key tile is wholly masked, the running maximum starts near -14427 (log2 units) and
    # jumps in the second tile; scattered masked prefix slots in the other sentence
    Case("masked_first_tile", B=2, S=30, P=100, NH=2, lengths=(30, 17),
         masked_prefix=tuple((0, s) for s in range(64)) + ((1, 0), (1, 5), (1, 63), (1, 64), (1, 99)), seed=7),
    # a sentence whose text is entirely masked while its prefix is live (the kernels run the full T there)
    Case("text_all_masked", B=2, S=20, P=4, NH=2, lengths=(20, 0), masked_prefix=((1, 1),), seed=8),
    # steep scores: Q and K times 3 (score standard deviation 9), three key tiles
    # (bf16 gradients: fp32-with-bf16-P measures 5.9e-3 norm / 6.2e-3 element-wise, bound 2.4e-2 / 2.5e-2: BF16_GRAD below)
    Case("steep_scaled", B=2, S=100, P=36, NH=2, lengths=(77, 100), qk_scale=3.0, seed=9),
    # ... and K rows scaled by a ramp along the key index, rising in sentence 0 and falling in sentence 1
    # (T = 192: three whole key tiles, so that the last one has as many candidates for the maximum as the others)
    # (bf16 gradients: fp32-with-bf16-P measures 8.0e-3 norm / 6.1e-3 element-wise, bound 3.2e-2 / 2.5e-2: BF16_GRAD below)
    Case("steep_ramp", B=2, S=130, P=62, NH=2, lengths=(130, 130), qk_scale=3.0, ramp=((0, 0.2, 3.0), (1, 3.0, 0.2)),
         holes=((1, 50),), seed=10),
    # every key of sentence 1 masked, P = 0: finite outputs and a context within rtol 5e-3 are all that is asked there
    Case("all_masked_p0", B=3, S=20, P=0, NH=2, lengths=(20, 0, 7), seed=11),
]
BY_NAME = {c.name: c for c in CASES}

# Seed and offset of every dropout launch of the GPU tests, and of the pricing below (the high word of the seed enters the key).
SEED, OFFSET = (3 << 32) + 5, 9

# bf16 gradients of the steep cases: (norm-relative bound, element-wise `close` rtol) in place of the defaults (1.2e-2, 2e-2).
# Their near-one-hot softmax makes dS = P (dPd - delta) a difference of nearly equal numbers.  Each bound is 4 x the error
# against float64 of the same formula in fp32 torch on bf16-valued inputs with P rounded to bf16 before P V (`priced_bf16_grad`:
# worst of dqkv / dpk / dpv over p in {0, 0.3}); test_attn_cases.py recomputes the measurement and holds the bounds to it.
#   steep_scaled: measured norm-relative 5.9e-3, element-wise 6.2e-3  -> 4 x = 2.4e-2, 2.5e-2
#   steep_ramp:   measured norm-relative 8.0e-3, element-wise 6.1e-3  -> 4 x = 3.2e-2, 2.5e-2
# Every other case measures at most 2.5e-3 / 3.3e-3: 4 x that is inside the defaults.
BF16_GRAD = {"steep_scaled": (2.4e-2, 2.5e-2), "steep_ramp": (3.2e-2, 2.5e-2)}


def mask_of(case):
    """[B, T] 1 = key takes part, 0 = masked."""
    m = torch.zeros(case.B, case.T)
    m[:, :case.P] = 1
    for b, n in enumerate(case.lengths):
        m[b, case.P:case.P + n] = 1
    for b, s in case.holes:
        assert s < case.lengths[b]
        m[b, case.P + s] = 0
    for b, s in case.masked_prefix:
        m[b, s] = 0
    return m


def last_unmasked(case):
    """Per sentence: the last unmasked text position, -1 when the text is entirely masked."""
    m = mask_of(case)[:, case.P:]
    return [int(torch.nonzero(m[b]).max()) if bool(m[b].any()) else -1 for b in range(case.B)]


def effective_T(case):
    """Per sentence: the key count the kernels loop over (trailing masked keys are skipped; the full T when no text key is live)."""
    return [case.P + l + 1 if l >= 0 else case.T for l in last_unmasked(case)]


def inputs(case, bf16=False, zero_tail=False):
    """qkv, pk, pv, addmask, mask, dctx as fp32 tensors (rounded to bf16 values when bf16).  dctx is dense and non-zero at every
    query; zero_tail zeroes it behind each sentence's last unmasked position (the contract of the tail variants, and what a
    packed launch cannot see)."""
    B, S, P, NH, H, T = case.B, case.S, case.P, case.NH, case.H, case.T
    g = torch.Generator().manual_seed(7000 + case.seed)
    qkv = torch.randn(B, S, 3, NH, D, generator=g)
    pk = torch.randn(B, NH, max(P, 1), D, generator=g)[:, :, :P]
    pv = torch.randn(B, NH, max(P, 1), D, generator=g)[:, :, :P]
    dctx = torch.randn(B, S, H, generator=g)
    qkv[:, :, 0] *= case.qk_scale
    qkv[:, :, 1] *= case.qk_scale
    pk = pk * case.qk_scale
    for b, f0, f1 in case.ramp:
        f = torch.linspace(f0, f1, T)
        pk[b] = pk[b] * f[:P].view(1, P, 1)
        qkv[b, :, 1] *= f[P:].view(S, 1, 1)
    if zero_tail:
        for b, l in enumerate(last_unmasked(case)):
            dctx[b, l + 1:] = 0.0
    mask = mask_of(case)
    out = dict(qkv=qkv.reshape(B * S, 3 * H), pk=pk.reshape(B, NH * P * D), pv=pv.reshape(B, NH * P * D),
               dctx=dctx.reshape(B * S, H), mask=mask, addmask=(1.0 - mask) * -10000.0)
    if bf16:
        for k in ("qkv", "pk", "pv", "dctx"):
            out[k] = out[k].to(torch.bfloat16).float()
    return out


def _heads(case, x):
    """qkv / pk / pv of `inputs` -> q [B,NH,S,D], k, v [B,NH,T,D] (prefix keys first)."""
    B, S, P, NH = case.B, case.S, case.P, case.NH
    q, k, v = (x["qkv"].view(B, S, 3, NH, D)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    if P:
        k = torch.cat([x["pk"].view(B, NH, P, D), k], 2)
        v = torch.cat([x["pv"].view(B, NH, P, D), v], 2)
    return q, k, v


def reference(case, keep=None, p=0.0, bf16=False, zero_tail=False):
    """Plain float64 torch.  -> dict(ctx, lse, probs, dqkv, dpk, dpv, delta): lse and probs are those of the UNdropped scores;
    with keep [B,NH,S,T] (0 / 1) the context is (probs * keep / (1 - p)) @ V.  Gradients of sum(ctx * dctx) by autograd through
    the float64 graph; delta = rowsum(dctx * ctx) per head.  Masked keys carry the additive -10000: exp of it is exactly 0 in
    float64 next to any live key, as in the kernels."""
    B, S, P, NH, H = case.B, case.S, case.P, case.NH, case.H
    x = inputs(case, bf16=bf16, zero_tail=zero_tail)
    leaves = {k: x[k].double().requires_grad_(True) for k in ("qkv", "pk", "pv")}
    q, k, v = _heads(case, leaves)
    s = q @ k.transpose(-1, -2) * SCALE + x["addmask"].double()[:, None, None, :]
    lse = torch.logsumexp(s, -1)
    probs = torch.exp(s - lse[..., None])
    pd = probs if keep is None else probs * torch.as_tensor(keep, dtype=torch.float64) / (1.0 - p)
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B * S, H)
    dctx = x["dctx"].double()
    (ctx * dctx).sum().backward()
    delta = (ctx.detach() * dctx).view(B, S, NH, D).sum(-1).permute(0, 2, 1)
    zero = torch.zeros(B, 0, dtype=torch.float64)
    return dict(ctx=ctx.detach(), lse=lse.detach(), probs=probs.detach(), dqkv=leaves["qkv"].grad,
                dpk=leaves["pk"].grad if P else zero, dpv=leaves["pv"].grad if P else zero, delta=delta.contiguous())


def closed_form(case, keep=None, p=0.0, bf16=False, zero_tail=False, dtype=torch.float64):
    """The same attention written out by hand in `dtype`, the way the kernels evaluate it: P = exp(S - lse), Pd = P * keep / (1-p),
    O = Pd V, dPd = dO V^T, delta = rowsum(dO * O), dS = P * (dPd * keep / (1-p) - delta) * scale, dQ = dS K, dK = dS^T Q,
    dV = Pd^T dO.  In float64 it checks the reference's autograd; in float32 it is the oracle's arithmetic, whose error against
    float64 prices a tolerance; with bf16 the inputs are bf16 values and Pd is rounded to bf16 before each product it enters
    (Pd V and Pd^T dO): nothing else is rounded."""
    B, S, P, NH, H, T = case.B, case.S, case.P, case.NH, case.H, case.T
    x = inputs(case, bf16=bf16, zero_tail=zero_tail)
    rb = (lambda t: t.to(torch.bfloat16).to(dtype)) if bf16 else (lambda t: t)
    q, k, v = (t.to(dtype) for t in _heads(case, x))
    s = q @ k.transpose(-1, -2) * SCALE + x["addmask"].to(dtype)[:, None, None, :]
    lse = torch.logsumexp(s, -1)
    probs = torch.exp(s - lse[..., None])
    kf = torch.ones(B, NH, S, T, dtype=dtype) if keep is None else torch.as_tensor(keep, dtype=dtype) / (1.0 - p)
    pd = rb(probs * kf)
    o = pd @ v                                                      # [B,NH,S,D]
    do = x["dctx"].to(dtype).view(B, S, NH, D).permute(0, 2, 1, 3)  # [B,NH,S,D]
    delta = (do * o).sum(-1)
    ds = probs * ((do @ v.transpose(-1, -2)) * kf - delta[..., None]) * SCALE
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, pd.transpose(-1, -2) @ do
    dqkv = torch.stack([dq, dk[:, :, P:], dv[:, :, P:]], 0).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * H)  # [3,B,NH,S,D] -> [B,S,3,NH,D]
    return dict(ctx=o.permute(0, 2, 1, 3).reshape(B * S, H), lse=lse, probs=probs, dqkv=dqkv,
                dpk=dk[:, :, :P].reshape(B, NH * P * D), dpv=dv[:, :, :P].reshape(B, NH * P * D), delta=delta)


# ---------------------------------------------------------------------------------------------------------
# measures, and the price of a bf16 gradient bound
# ---------------------------------------------------------------------------------------------------------
def need(got, ref):
    """The smallest rtol at which `close` of test_ops_gpu.py passes (its absolute term: rtol * max |ref| + 1e-7)."""
    got, ref = got.double().cpu(), ref.double()
    if ref.numel() == 0:
        return 0.0
    err = ((got - ref).abs() - 1e-7).clamp_min(0.0)
    return float((err / (ref.abs().max() + ref.abs()).clamp_min(1e-300)).max())


def relerr(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm()) if ref.numel() else 0.0


def priced_bf16_grad(case):
    """(norm-relative, element-wise) error against float64 of the fp32 evaluation with P rounded to bf16, over the sentences that
    are compared: the worst of dqkv / dpk / dpv over p in {0, 0.3}."""
    worst = [0.0, 0.0]
    live = [b for b in range(case.B) if b not in case.exempt]
    for p in (0.0, 0.3):
        keep = keep_mask(SEED, OFFSET, case.B, case.NH, case.S, case.T, p) if p else None
        ref = reference(case, keep=keep, p=p, bf16=True)
        got = closed_form(case, keep=keep, p=p, bf16=True, dtype=torch.float32)
        for k in ("dqkv", "dpk", "dpv"):
            g, r = got[k].reshape(case.B, -1)[live], ref[k].reshape(case.B, -1)[live]
            worst = [max(worst[0], relerr(g, r)), max(worst[1], need(g, r))]
    return tuple(worst)


# ---------------------------------------------------------------------------------------------------------
# the dropout decision (csrc/common.h: mix32, attn_dropout_rowhash, attn_dropout_keep2; csrc/attention_args.h: attn_drop_key,
# attn_drop_thr) in numpy uint32.  Valid only while no device epoch word is registered (the epoch is folded into the key).
# ---------------------------------------------------------------------------------------------------------
_M = 0xFFFFFFFF


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M
    x ^= x >> np.uint64(16)
    return x


def drop_key(seed, offset):
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    inner = _mix32((offset & _M) ^ 0x9E3779B9)
    mid = _mix32(np.uint64(seed >> 32) ^ inner)
    return int(_mix32(np.uint64(seed & _M) ^ mid))


def drop_thr(p):
    return int(min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0))) if p > 0 else 0


def keep_mask(seed, offset, B, NH, S, T, p):
    """[B, NH, S, T] bool: True where the kernels keep the probability of (sentence b, head h, query q, key t).
    row = (b*NH + h)*S + q, col = t, keep <=> ((mix32(row * 0x9E3779B1 + key) ^ (col * 0x85EBCA77)) * 0x2c1b3c6d mod 2^32) >= thr."""
    key = np.uint64(drop_key(seed, offset))
    row = np.arange(B * NH * S, dtype=np.uint64)
    rowh = _mix32((row * np.uint64(0x9E3779B1) + key) & _M)
    cterm = (np.arange(T, dtype=np.uint64) * np.uint64(0x85EBCA77)) & _M
    val = ((rowh[:, None] ^ cterm[None, :]) * np.uint64(0x2C1B3C6D)) & _M
    return (val >= np.uint64(drop_thr(p))).reshape(B, NH, S, T)


# ---------------------------------------------------------------------------------------------------------
# packed rows of a suffix-masked case
# ---------------------------------------------------------------------------------------------------------
def kept_rows(case):
    """Row indices into the padded [B*S] token axis of the unmasked tokens, sentence after sentence."""
    assert case.suffix_masked
    return torch.tensor([b * case.S + s for b, n in enumerate(case.lengths) for s in range(n)])


def cu_plain(case):
    """cu [B+1] int32: sentence b owns packed rows cu[b] .. cu[b+1]-1."""
    assert case.suffix_masked
    return torch.tensor(np.concatenate([[0], np.cumsum(case.lengths)]), dtype=torch.int32)


def cu_ordered(case):
    """cu [2B+1] int32 of the ordered launch: cu[0] = -1 marks the list (row 0 is sentence 0's either way), cu[1..B] the offsets,
    cu[B+1+z] the sentence that grid slot z runs -- longest first, ties by index."""
    cu = cu_plain(case)
    order = sorted(range(case.B), key=lambda b: (-case.lengths[b], b))
    out = torch.cat([cu, torch.tensor(order, dtype=torch.int32)])
    out[0] = -1
    return out
