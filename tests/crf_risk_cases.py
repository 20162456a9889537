"""Inputs, references and bounds shared by the tests of the expected-cost (risk) entry points (test_crf_risk.py on the CPU,
test_crf_risk_gpu.py on the GPU): mtvaf_crf_risk_{fwd,bwd} and the layers above them.

Reference: float64 autograd.  logZ from crf_lattice_cases.log_partition without sets, marg = d logZ / d em with create_graph,
R[b] = sum over the live columns of marg * cost, every gradient from autograd.grad((R * w).sum(), ...) -- a double backward
through the Python loop over columns.  test_crf_risk.py pins it against enumeration of all paths.

Error model: ``centred`` below, a torch restatement of the centred recursions of csrc/crf_risk.hip's header (normalised
alphas, the cost-weighted chains re-centred at every step, R summed on its own), run in float32.  It is what a correct
single-precision implementation can reach; float32 autograd double-backward is NOT (its error grows with len |cost|: 11 % of
max|dR/dem| at S = 512), so it is not used here.  Run in float64, the same code agrees with the autograd reference to
rounding, which test_crf_risk.py checks too.

Acceptance rule: |got - ref64| <= max(T_proj, 4 max|centred32 - ref64|), T_proj = 2e-5 max|ref| for risk and logz, 1e-4 max|ref|
+ 1e-7 for marg, dem, dstart, dend, dtrans, dcost (the rule of crf_llh_cases).  Against a vacuous bound, make_reference asserts
that every bound is at most 1e-3 max|ref64| + 1e-7."""
import functools
import types

import torch

import crf_lattice_cases as X
import crf_llh_cases as L

SHAPES = [(1, 1, 1, 1), (3, 2, 2, 1), (70, 1, 2, 1), (3, 17, 11, 1), (70, 17, 16, 1), (3, 65, 11, 1), (3, 65, 11, 6),
          (1, 2, 16, 1), (3, 17, 17, 1), (1, 65, 64, 1), (3, 2, 64, 1), (3, 512, 64, 1)]
# cost patterns: (h) Hamming against the case's tags, (r) signed randn, (z) zeros, (k) a per-column constant plus (r), (n) (r)
# with NaN at the masked columns
PATTERNS = ("h", "r", "z", "k", "n")
QUANTITIES = ("risk", "logz", "marg", "dem", "dstart", "dend", "dtrans", "dcost")
BRUTE = X.BRUTE


def live(mask):
    """bool [B,S]: the columns before each sentence's length."""
    return torch.arange(mask.shape[1])[None] < X.lengths_of(mask)[:, None]


def column_constants(shape):
    B, S, _, _ = shape
    return 3.0 * torch.randn(B, S, 1, generator=torch.Generator().manual_seed(77 + sum(shape)))


def make_cost(shape, pattern, inp):
    em, tags, mask, *_ = inp
    B, S, C = em.shape
    if pattern == "h":
        return (1.0 - torch.nn.functional.one_hot(tags, C).float()) * live(mask)[..., None]
    if pattern == "z":
        return torch.zeros(B, S, C)
    r = torch.randn(B, S, C, generator=torch.Generator().manual_seed(53 + sum(shape)))
    if pattern == "r":
        return r
    if pattern == "k":
        return r + column_constants(shape)
    if pattern == "n":
        return torch.where(live(mask)[..., None], r, torch.full_like(r, float("nan")))
    raise ValueError(pattern)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def oracle(inp, cost, w, dtype=torch.float64):
    em, _, mask, start, end, trans = inp
    on = live(mask)[..., None]
    em_, s_, e_, t_ = (x.to(dtype).clone().requires_grad_(True) for x in (em, start, end, trans))
    c_ = torch.where(on, cost.to(dtype), torch.zeros((), dtype=dtype)).requires_grad_(True)
    logz = X.log_partition(em_, None, mask, s_, e_, t_)
    marg, = torch.autograd.grad(logz.sum(), em_, create_graph=True)
    risk = (marg * c_ * on).sum((1, 2))
    grads = torch.autograd.grad((risk * w.to(dtype)).sum(), [em_, s_, e_, t_, c_], allow_unused=True)  # (S = 1: no transition)
    dem, dstart, dend, dtrans, dcost = (torch.zeros_like(p) if g is None else g for g, p in zip(grads, (em_, s_, e_, t_, c_)))
    return dict(risk=risk.detach(), logz=logz.detach(), marg=(marg * on).detach(), dem=dem * on, dstart=dstart, dend=dend,
                dtrans=dtrans, dcost=dcost * on)


# ---- the centred recursions --------------------------------------------------------------------------------------------------
def centred(inp, cost, w, dtype=torch.float32):
    """Every quantity of ``oracle`` by the centred recursions, sentence by sentence, in ``dtype``."""
    em, _, mask, start, end, trans = (x if x.dtype in (torch.uint8, torch.int64, torch.bool) else x.to(dtype) for x in inp)
    cost, w = cost.to(dtype), w.to(dtype)
    B, S, C = em.shape
    lens = X.lengths_of(mask)
    out = dict(risk=torch.zeros(B, dtype=dtype), logz=torch.zeros(B, dtype=dtype), marg=torch.zeros(B, S, C, dtype=dtype),
               dem=torch.zeros(B, S, C, dtype=dtype), dcost=torch.zeros(B, S, C, dtype=dtype), dstart=torch.zeros(C, dtype=dtype),
               dend=torch.zeros(C, dtype=dtype), dtrans=torch.zeros(C, C, dtype=dtype))
    tmax = trans.max()
    E = torch.exp(trans - tmax)
    for b in range(B):
        n = int(lens[b])
        e, c = em[b, :n], cost[b, :n]
        mx = e.max(1).values
        # forward: abar_t the normalised alpha, at_t = cost_t + sum_i w_t(i->j) ac_{t-1}(i), ac_t = at_t - mean_t
        abar, sp, ac, mean = [None] * n, [None] * n, [None] * n, [None] * n
        a0 = start + e[0]
        s = torch.exp(a0 - a0.max())
        lz = a0.max() + torch.log(s.sum())
        abar[0] = s / s.sum()
        at = c[0]
        for t in range(n):
            if t >= 1:
                sp[t] = abar[t - 1] @ E
                at = c[t] + ((abar[t - 1] * ac[t - 1]) @ E) / sp[t]
                s = sp[t] * torch.exp(e[t] - mx[t])
                lz = lz + tmax + mx[t] + torch.log(s.sum())
                abar[t] = s / s.sum()
            mean[t] = (abar[t] * at).sum()
            ac[t] = at - mean[t]
        pe = abar[n - 1] * torch.exp(end - end.max())
        out["logz"][b] = lz + end.max() + torch.log(pe.sum())
        pe = pe / pe.sum()
        out["risk"][b] = (torch.stack(mean).double().sum() + (pe * ac[n - 1]).sum().double()).to(dtype)
        # backward: bt the scaled beta, bh = bc_t; d_t = ac_t + bc_t, dbar_t its mean under the node marginal
        bt, bh = torch.exp(end - end.max()), torch.zeros(C, dtype=dtype)
        G = torch.zeros(C, C, dtype=dtype)
        val = [None] * n
        for t in range(n - 1, 0, -1):
            u = torch.exp(e[t] - mx[t]) * bt
            d = (sp[t] * u).sum()
            ui = u / d
            mu = sp[t] * ui
            q = u * (c[t] + bh)
            eu, eq, dq = E @ u, E @ q, (sp[t] * q).sum()
            dv = ac[t] + bh
            dbar = (mu * dv).sum()
            val[t] = mu * (dv - dbar)
            out["marg"][b, t] = mu
            k = ui * (c[t] + bh - dbar - mean[t])
            G = G + torch.outer(abar[t - 1] * ac[t - 1], ui) + torch.outer(abar[t - 1], k)
            bt, bh = eu / d, eq / eu - dq / d
        p0 = abar[0] * bt
        p0 = p0 / p0.sum()
        dv = ac[0] + bh
        val[0] = p0 * (dv - (p0 * dv).sum())
        out["marg"][b, 0] = p0
        out["dem"][b, :n] = w[b] * torch.stack(val)
        out["dcost"][b, :n] = w[b] * out["marg"][b, :n]
        out["dstart"] += w[b] * val[0]
        out["dend"] += w[b] * val[n - 1]
        out["dtrans"] += w[b] * G * E
    return out


def bound(name, r64, c32):
    t_proj = 2e-5 * float(r64.abs().max()) if name in ("risk", "logz") else 1e-4 * float(r64.abs().max()) + 1e-7
    return max(t_proj, 4.0 * float((c32.double() - r64).abs().max()))


def make_reference(inp, cost, w=None):
    w = L.weights(inp[0].shape[0]) if w is None else w
    r64, c32 = oracle(inp, cost, w), centred(inp, cost, w)
    bnd = {k: bound(k, r64[k], c32[k]) for k in QUANTITIES}
    for k in QUANTITIES:  # (a bound that an error model gone wrong has blown up would accept anything)
        assert bnd[k] <= 1e-3 * float(r64[k].abs().max()) + 1e-7, f"vacuous bound for {k}: {bnd[k]:.3e}"
    return types.SimpleNamespace(inputs=inp, cost=cost, w=w, r64=r64, c32=c32, bound=bnd)


@functools.lru_cache(maxsize=None)
def reference(shape, pattern):
    """Inputs, cost, float64 reference, centred float32 restatement and bounds of one case: computed once, shared, not to be
    modified.  Pattern (n) has no reference of its own (its outputs are (r)'s bit for bit)."""
    assert pattern in ("h", "r", "z", "k")
    inp = X.inputs(shape)
    return make_reference(inp, make_cost(shape, pattern, inp))


WORST = {}


def check(ref, name, got, add=None, bound_name=None):
    """Assert ``got`` against the float64 reference (plus ``add``, for accumulated gradients); prints err / bound."""
    r64 = ref.r64[name] if add is None else ref.r64[name] + add
    bnd = ref.bound[bound_name or name]
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    err = float((got - r64).abs().max())
    r = err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf"))  # (a reference that is identically 0, met exactly)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"crf-risk ratio {name} {r:.4f} (err {err:.3e}, bound {bnd:.3e}; worst so far {WORST[name]:.4f})")
    assert r <= 1.0, f"{name}: err / bound = {r:.3f}"


def bruteforce(inp, cost, w):
    """risk [B], dem [B,S,C], dtrans [C,C] of sum_b w[b] R[b] in float64 by enumerating all C^L paths:
    dR/dem[t,c] = sum_y p(y) [y_t = c] (cost(y) - R),  dR/dtrans[i,j] = sum_y p(y) #{t: y_{t-1} = i, y_t = j} (cost(y) - R)."""
    em, _, mask, start, end, trans = inp
    emd, sd, ed, td, cd, wd = (x.double() for x in (em, start, end, trans, cost, w))
    B, S, C = em.shape
    risk, dem, dtrans = torch.zeros(B, dtype=torch.float64), torch.zeros(B, S, C, dtype=torch.float64), \
        torch.zeros(C, C, dtype=torch.float64)
    for b in range(B):
        n = int(X.lengths_of(mask)[b])
        paths = torch.cartesian_prod(*[torch.arange(C)] * n).reshape(-1, n)
        sc = sd[paths[:, 0]] + emd[b, 0, paths[:, 0]] + ed[paths[:, -1]]
        cy = cd[b, 0, paths[:, 0]]
        for t in range(1, n):
            sc = sc + td[paths[:, t - 1], paths[:, t]] + emd[b, t, paths[:, t]]
            cy = cy + cd[b, t, paths[:, t]]
        p = torch.exp(sc - torch.logsumexp(sc, 0))
        risk[b] = (p * cy).sum()
        dev = p * (cy - risk[b])
        for t in range(n):
            dem[b, t].index_add_(0, paths[:, t], wd[b] * dev)
            if t >= 1:
                dtrans.view(-1).index_add_(0, paths[:, t - 1] * C + paths[:, t], wd[b] * dev)
    return risk, dem, dtrans
