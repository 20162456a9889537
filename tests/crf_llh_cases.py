"""Inputs, references and the acceptance rule shared by the tests of the per-sentence CRF likelihoods and the tag
marginals (test_crf_llh.py on the CPU, test_crf_llh_gpu.py on the GPU).

Reference: the float64 oracle -- ``O.crf_log_likelihood(..., "none")`` and float64 autograd through it; the marginals
are float64 autograd of ``O.crf_log_partition(...).sum()`` with respect to the emissions (zero at masked steps).

Acceptance rule, one for likelihoods, gradients and marginals: an element passes if
    |got - ref64| <= max(T_proj, 4 * max|ref32 - ref64|)
where ref32 is the same oracle run in float32 on the same inputs and T_proj is the bound of the existing CRF tests
(``close()`` of test_crf_wide_gpu.py): 2e-5 * max|ref| for likelihoods, 1e-4 * max|ref| + 1e-7 for gradients and
marginals.  The factor 4 over the float32 reference's own error is there because the kernels work in the scaled linear
domain, with a different rounding order than the log-domain oracle.  The float32 reference alone always meets the rule.

One degenerate corner: with a single tag (C = 1) every path is the gold path, so llh = score - logZ is identically 0 in
float64 and, in a third of these cases, in the float32 oracle too (it sums both terms in the same order) -- the rule as
stated gives the bound 0 there, which no float32 difference of two separately rounded sums of size |logZ| can be held to.
For a likelihood whose float64 reference is identically zero, and only then, T_proj takes its scale from the terms of the
difference: 2e-5 * max|logZ|.  Every other case and quantity uses the rule exactly as stated above.
"""
import functools
import types

import torch

import crf_wide_cases as W
from oracle import mtvaf_oracle as O

# (B, S, C, scale) as crf_wide_cases.fixed_case reads them: scale > 1 spreads the scores over tens of nats, scale < 0
# punches holes in the mask.  Narrow path (C <= 16): C = 1 and 2 are the degenerate tag sets, 11 the model's, 16 fills the
# DPP row; S = 16 / 17 straddle the 16-row LDS rounding, 65 the 64-step mask word; B = 70 crosses the 64-wide strides of
# the reductions.
NARROW = [(B, S, C, 1) for C in (1, 2, 11, 16) for S in (1, 2, 16, 17, 65) for B in (1, 3, 70)] + \
         [(3, 65, 11, -1), (3, 65, 11, 6)]
# wide path (17 <= C <= 64), from crf_wide_cases.FIXED: the smallest, S = 1, holes, large magnitudes, the S limit
WIDE = [(4, 5, 17, 1), (2, 1, 64, 1), (4, 66, 48, -1), (6, 128, 64, 6), (3, 512, 64, 1)]
assert all(c in W.FIXED for c in WIDE)
CASES = NARROW + WIDE
# brute-force known answers: (B, S, C, seed, lengths)
BRUTE = [(3, 4, 5, 76, [4, 2, 1])] + list(W.BRUTE)

QUANTITIES = ("llh", "logz", "marg", "dem", "dstart", "dend", "dtrans")
LIKELIHOODS = ("llh", "logz")


def weights(B, seed=11):
    """Per-sentence upstream gradients of mixed sign; from two sentences on, one of them is an exact 0."""
    w = torch.randn(B, generator=torch.Generator().manual_seed(seed + B)) * 1.5
    w[0] = w[0].abs() + 0.25
    if B >= 2:
        w[1] = 0.0
    if B >= 3:
        w[-1] = -w[-1].abs() - 0.25
    return w


def oracle(inputs, w, dtype):
    """Every quantity the kernels produce, from the oracle in ``dtype``."""
    em, tags, mask, start, end, trans = inputs
    em_, s_, e_, t_ = (x.to(dtype).clone().requires_grad_(True) for x in (em, start, end, trans))
    logz = O.crf_log_partition(em_, mask, s_, e_, t_)
    marg, = torch.autograd.grad(logz.sum(), em_)
    llh = O.crf_log_likelihood(em_, tags, mask, s_, e_, t_, "none")
    grads = torch.autograd.grad((llh * w.to(dtype)).sum(), [em_, s_, e_, t_], allow_unused=True)
    dem, dstart, dend, dtrans = (torch.zeros_like(p) if g is None else g for g, p in zip(grads, (em_, s_, e_, t_)))
    return dict(llh=llh.detach(), logz=logz.detach(), marg=marg, dem=dem, dstart=dstart, dend=dend, dtrans=dtrans)


def bound(name, ref64, ref32, logz64=None):
    m = float(ref64.abs().max())
    if m == 0.0 and name in LIKELIHOODS and logz64 is not None:
        m = float(logz64.abs().max())  # (C = 1: llh is identically zero; module docstring)
    t_proj = 2e-5 * m if name in LIKELIHOODS else 1e-4 * m + 1e-7
    return max(t_proj, 4.0 * float((ref32.double() - ref64).abs().max()))


def make_reference(inputs):
    w = weights(inputs[0].shape[0])
    r64, r32 = oracle(inputs, w, torch.float64), oracle(inputs, w, torch.float32)
    return types.SimpleNamespace(inputs=inputs, w=w, r64=r64, r32=r32,
                                 bound={k: bound(k, r64[k], r32[k], r64["logz"]) for k in QUANTITIES})


@functools.lru_cache(maxsize=None)
def reference(case):
    """The inputs of ``case`` with their float64 / float32 references and bounds: computed once, shared, not to be modified."""
    return make_reference(W.fixed_case(*case))


def ratio(name, got, ref64, bnd):
    """max|got - ref64| / bound; the tests assert <= 1 and print it (the largest per quantity goes into DESIGN.md)."""
    err = float((torch.as_tensor(got).detach().double().cpu() - ref64).abs().max())
    r = err / bnd
    print(f"crf-llh ratio {name} {r:.4f} (err {err:.3e}, bound {bnd:.3e})")
    return r


def check(ref, name, got, add=None):
    """Assert ``got`` against the float64 reference of quantity ``name`` (plus ``add``, for accumulated gradients)."""
    r64 = ref.r64[name] if add is None else ref.r64[name] + add
    r = ratio(name, got, r64, ref.bound[name])
    assert r <= 1.0, f"{name}: err / bound = {r:.3f}"


def bruteforce(em, tags, mask, start, end, trans):
    """llh [B], logZ [B] and node marginals [B,S,C] in float64 by enumerating all C^L paths (contiguous masks)."""
    emd, sd, ed, td = (x.double() for x in (em, start, end, trans))
    B, S, C = em.shape
    llh, logz, marg = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), \
        torch.zeros(B, S, C, dtype=torch.float64)
    for b in range(B):
        L = int(mask[b].long().sum())
        assert bool(mask[b, :L].all())
        paths = torch.cartesian_prod(*[torch.arange(C)] * L).reshape(-1, L)  # [C^L, L]
        sc = sd[paths[:, 0]] + emd[b, 0, paths[:, 0]] + ed[paths[:, -1]]
        for t in range(1, L):
            sc = sc + td[paths[:, t - 1], paths[:, t]] + emd[b, t, paths[:, t]]
        logz[b] = torch.logsumexp(sc, 0)
        p = torch.exp(sc - logz[b])
        for t in range(L):
            marg[b, t].index_add_(0, paths[:, t], p)
        gold = tags[b, :L]
        llh[b] = sc[int((paths == gold[None]).all(1).nonzero()[0])] - logz[b]
    return llh, logz, marg


@functools.lru_cache(maxsize=None)
def brute_reference(case):
    B, S, C, seed, lengths = case
    inputs = W.crf_inputs(B, S, C, seed, lengths=list(lengths))
    ref = make_reference(inputs)
    ref.brute = dict(zip(("llh", "logz", "marg"), bruteforce(*inputs)))
    return ref


BRUTE = [(B, S, C, seed, tuple(lengths)) for B, S, C, seed, lengths in BRUTE]  # (hashable: brute_reference caches on it)
