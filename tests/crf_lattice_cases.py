"""Inputs, references and bounds shared by the tests of the constrained CRF entry points (test_crf_lattice.py on the CPU,
test_crf_lattice_gpu.py on the GPU): mtvaf_crf_lattice_{fwd,bwd,marginals,viterbi} and the layers above them.

Reference: a log-domain forward recursion in torch over the per-position tag sets (disallowed tags carry -inf), run in
float64 (and in float32 for the acceptance rule), autograd for the constrained posteriors and every gradient; a float64
Viterbi in numpy with the tie rule of the contract (the lowest allowed previous tag, at the end the lowest allowed last tag)
and mtvaf_crf_viterbi's order of additions.  test_crf_lattice.py pins both against enumeration of all paths and against the
unconstrained oracle.

Acceptance rule: the one of crf_llh_cases (``bound``), |got - ref64| <= max(T_proj, 4 max|ref32 - ref64|), with T_proj =
2e-5 max|ref| for logz_a / logz, 1e-4 max|ref| + 1e-7 for posteriors and gradients, and for pllh -- a difference of two
log-partitions that can be near 0 while its terms are large -- T_proj = 2e-5 max|logZ|, the scale of the terms of the
difference, as that file's C = 1 provision."""
import functools
import types

import numpy as np
import torch

import crf_llh_cases as L
import crf_wide_cases as W

# (B, S, C, scale): C = 1, 2 degenerate, 11 the model's, 16 / 17 the first width's edge, 64 the last lane; S = 1, 2 the
# recursion's ends, 17 / 65 odd lengths past the 16- and 64-column strides, 512 the limit; B = 70 more sentences than lanes
# in the reductions over sentences; scale 6 spreads the scores over tens of nats.
SHAPES = [(1, 1, 1, 1), (3, 2, 2, 1), (70, 1, 2, 1), (3, 17, 11, 1), (70, 17, 16, 1), (3, 65, 11, 1), (3, 65, 11, 6),
          (1, 2, 16, 1), (3, 17, 17, 1), (3, 65, 17, 1), (1, 65, 64, 1), (3, 2, 64, 1), (3, 512, 64, 1)]
# set patterns: (a) all full, (b) singletons {gold}, (c) random sets of density 1/2 around a random gold path, (d)
# structural_sets of a synthetic label map, (e) zero words and words of garbage bits >= C (must equal (a) bit for bit), (f) the
# sets of (c) with the emissions of the allowed tags 120 nats below the others at every column
PATTERNS = ("a", "b", "c", "d", "e", "f")
BRUTE = [(3, 4, 5, 76, (4, 2, 1))] + [(B, S, C, seed, tuple(lengths)) for B, S, C, seed, lengths in W.BRUTE]
QUANTITIES = ("pllh", "logz_a", "logz", "marg", "dem", "dstart", "dend", "dtrans")


def to_word(bits):
    """bool [..., C] -> int64 set words (bit 63 lands in the sign)."""
    C = bits.shape[-1]
    w = torch.zeros(bits.shape[:-1], dtype=torch.int64)
    for j in range(C):
        v = (1 << j) - (1 << 64) if j == 63 else 1 << j
        w |= torch.where(bits[..., j], torch.tensor(v, dtype=torch.int64), torch.tensor(0, dtype=torch.int64))
    return w


def effective_sets(allowed, C):
    """int64 [B,S] -> bool [B,S,C]: the low C bits, and the full set where none of them is set."""
    m = ((allowed[..., None] >> torch.arange(C)) & 1).bool()
    m[~m.any(-1)] = True
    return m


def lengths_of(mask):
    return torch.cumprod(mask.long(), dim=1).sum(1)


def label_map(C):
    """A label map over ids 1 .. C-1 (0 is PAD) in the reference's style, as far as C reaches."""
    names = ["O", "X", "[CLS]", "[SEP]"] + [f"{k}-T{i}" for i in range(32) for k in ("B", "I")]
    return {n: i for i, n in enumerate(names[:C - 1], 1)} if C > 1 else {"O": 0}


def inputs(shape):
    """em, tags, mask, start, end, trans: a prefix mask with ragged lengths, the first sentence full, the last of length 1."""
    B, S, C, scale = shape
    g = torch.Generator().manual_seed(17 + 7 * B + 31 * S + 1009 * C)
    lengths = [S] + [int(x) for x in torch.randint(1, S + 1, (B - 1,), generator=g)]
    if B >= 2:
        lengths[-1] = 1
    em, tags, mask, start, end, trans = W.crf_inputs(B, S, C, 3 + S + 1000 * C, lengths=lengths)
    if scale > 1:
        em, trans = em * scale, trans * 4 * scale
    return em, tags, mask, start, end, trans


def exact_inputs(shape):
    """The same layout with emissions, start, end, trans integers in [-16, 16] divided by 8: every partial sum of a path score
    is exact in float32, and equal scores are frequent -- the test of the tie rule."""
    em, tags, mask, start, end, trans = inputs(shape)
    g = torch.Generator().manual_seed(29 + sum(shape))
    q = lambda x: torch.randint(-16, 17, x.shape, generator=g).float() / 8
    return q(em), tags, mask, q(start), q(end), q(trans)


def sets(shape, pattern, inp):
    """-> (allowed int64 [B,S], emissions): the pattern's set words and the emissions to use with them."""
    em, tags, mask, *_ = inp
    B, S, C = em.shape
    g = torch.Generator().manual_seed(41 + sum(shape[:3]) + ord(pattern))
    full = torch.ones(B, S, C, dtype=torch.bool)
    if pattern == "a":
        return to_word(full), em
    if pattern == "b":
        return to_word(torch.nn.functional.one_hot(tags, C).bool()), em
    if pattern in ("c", "f"):
        gold = torch.randint(0, C, (B, S), generator=g)
        bits = (torch.rand(B, S, C, generator=g) < 0.5) | torch.nn.functional.one_hot(gold, C).bool()
        if pattern == "f":
            em = em - 120.0 * bits.float()
        return to_word(bits), em
    if pattern == "d":
        from mtvaf_amd.constraints import structural_sets
        words = torch.rand(B, S, generator=g) < 0.7
        return structural_sets(label_map(C), mask, words), em
    if pattern == "e":
        junk = torch.randint(0, 1 << 30, (B, S), generator=g) << min(C, 63)
        if C == 64:
            junk = torch.zeros_like(junk)
        return torch.where(torch.rand(B, S, generator=g) < 0.5, junk, torch.zeros_like(junk)), em
    raise ValueError(pattern)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def log_partition(em, sets_, mask, start, end, trans):
    """log sum over the paths inside ``sets_`` (bool [B,S,C]; None: all paths) of exp score(y), [B]; prefix masks."""
    B, S, C = em.shape
    if sets_ is not None:
        em = torch.where(sets_, em, torch.full_like(em, float("-inf")))
    score = start[None] + em[:, 0]
    for t in range(1, S):
        nxt = torch.logsumexp(score[:, :, None] + trans[None], dim=1) + em[:, t]
        score = torch.where(mask[:, t, None].bool(), nxt, score)
    return torch.logsumexp(score + end[None], dim=1)


def oracle(em, allowed, mask, start, end, trans, w, dtype):
    C = em.shape[2]
    A = effective_sets(allowed, C)
    em_, s_, e_, t_ = (x.to(dtype).clone().requires_grad_(True) for x in (em, start, end, trans))
    logz_a = log_partition(em_, A, mask, s_, e_, t_)
    logz = log_partition(em_, None, mask, s_, e_, t_)
    pllh = logz_a - logz
    marg, = torch.autograd.grad(logz_a.sum(), em_, retain_graph=True)
    grads = torch.autograd.grad((pllh * w.to(dtype)).sum(), [em_, s_, e_, t_], allow_unused=True)  # (S = 1: no transition)
    dem, dstart, dend, dtrans = (torch.zeros_like(p) if g is None else g for g, p in zip(grads, (em_, s_, e_, t_)))
    on = (torch.arange(em.shape[1])[None] < lengths_of(mask)[:, None])[..., None]
    return dict(pllh=pllh.detach(), logz_a=logz_a.detach(), logz=logz.detach(), marg=marg * on, dem=dem * on, dstart=dstart,
                dend=dend, dtrans=dtrans)


def bound(name, r64, r32):
    if name == "pllh":  # (T_proj from the terms of the difference: module docstring)
        return max(2e-5 * float(r64["logz"].abs().max()), 4.0 * float((r32["pllh"].double() - r64["pllh"]).abs().max()))
    return L.bound("logz" if name in ("logz_a", "logz") else name, r64[name], r32[name])


def make_reference(inp, allowed):
    em, tags, mask, start, end, trans = inp
    w = L.weights(em.shape[0])
    r64 = oracle(em, allowed, mask, start, end, trans, w, torch.float64)
    r32 = oracle(em, allowed, mask, start, end, trans, w, torch.float32)
    return types.SimpleNamespace(inputs=inp, allowed=allowed, sets=effective_sets(allowed, em.shape[2]), w=w, r64=r64, r32=r32,
                                 bound={k: bound(k, r64, r32) for k in QUANTITIES})


@functools.lru_cache(maxsize=None)
def reference(shape, pattern):
    """Inputs, sets, float64 / float32 references and bounds of one case: computed once, shared, not to be modified."""
    inp = inputs(shape)
    allowed, em = sets(shape, pattern, inp)
    return make_reference((em,) + inp[1:], allowed)


WORST = {}


def check(ref, name, got, add=None):
    """Assert ``got`` against the float64 reference (plus ``add``, for accumulated gradients); prints err / bound."""
    r64 = ref.r64[name] if add is None else ref.r64[name] + add
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    r = float((got - r64).abs().max()) / ref.bound[name]
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"crf-lattice ratio {name} {r:.4f} (bound {ref.bound[name]:.3e}; worst so far {WORST[name]:.4f})")
    assert r <= 1.0, f"{name}: err / bound = {r:.3f}"


def viterbi(em, allowed, mask, start, end, trans):
    """float64 Viterbi over the allowed paths -> (tags [B,S] int64 padded with -1, lengths [B], scores [B] float64)."""
    B, S, C = em.shape
    A = effective_sets(allowed, C).numpy()
    e, s0, e1, tr = (x.double().numpy() for x in (em, start, end, trans))
    lens = lengths_of(mask).numpy()
    tags, scores = np.full((B, S), -1, dtype=np.int64), np.zeros(B)
    for b in range(B):
        n = int(lens[b])
        score = np.where(A[b, 0], s0 + e[b, 0], -np.inf)
        back = np.zeros((n, C), dtype=np.int64)
        for t in range(1, n):
            cand = score[:, None] + tr            # [previous, next]
            back[t] = cand.argmax(0)              # (the first maximum: the lowest previous tag; disallowed ones hold -inf)
            score = np.where(A[b, t], cand.max(0) + e[b, t], -np.inf)
        fin = score + e1
        cur = int(fin.argmax())
        scores[b] = fin[cur]
        for t in range(n - 1, -1, -1):
            tags[b, t] = cur
            cur = int(back[t, cur])
    return torch.from_numpy(tags), torch.from_numpy(lens), torch.from_numpy(scores)


def path_score(em, tags, mask, start, end, trans):
    """float64 score of the given paths [B,S] (entries behind the length ignored), [B]."""
    e, s0, e1, tr = (x.double() for x in (em, start, end, trans))
    lens = lengths_of(mask)
    out = torch.zeros(em.shape[0], dtype=torch.float64)
    for b in range(em.shape[0]):
        p = tags[b, :int(lens[b])].long()
        sc = s0[p[0]] + e[b, 0, p[0]] + e1[p[-1]]
        if len(p) > 1:
            sc = sc + tr[p[:-1], p[1:]].sum() + e[b, torch.arange(1, len(p)), p[1:]].sum()
        out[b] = sc
    return out


def bruteforce(em, allowed, mask, start, end, trans):
    """logZ_A [B], logZ [B] and the constrained posteriors [B,S,C] in float64 by enumerating all C^L paths and keeping the
    allowed ones."""
    emd, sd, ed, td = (x.double() for x in (em, start, end, trans))
    B, S, C = em.shape
    A = effective_sets(allowed, C)
    logz_a, logz, marg = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), \
        torch.zeros(B, S, C, dtype=torch.float64)
    for b in range(B):
        n = int(lengths_of(mask)[b])
        paths = torch.cartesian_prod(*[torch.arange(C)] * n).reshape(-1, n)
        sc = sd[paths[:, 0]] + emd[b, 0, paths[:, 0]] + ed[paths[:, -1]]
        ok = A[b, 0, paths[:, 0]]
        for t in range(1, n):
            sc = sc + td[paths[:, t - 1], paths[:, t]] + emd[b, t, paths[:, t]]
            ok = ok & A[b, t, paths[:, t]]
        logz[b] = torch.logsumexp(sc, 0)
        logz_a[b] = torch.logsumexp(sc[ok], 0)
        p = torch.exp(sc[ok] - logz_a[b])
        for t in range(n):
            marg[b, t].index_add_(0, paths[ok][:, t], p)
    return logz_a, logz, marg
