"""Inputs, references and bounds shared by the tests of the path-cost entry points (test_crf_path.py on the CPU,
test_crf_path_gpu.py on the GPU): mtvaf_crf_path_{fwd,bwd} and the layers above them (expected_path_cost, entropy, kl_divergence).

Reference: float64 autograd.  ``expect`` forms R[b] = sum_t sum_c m_t(c) cost[b,t,c] + sum_t sum_ij xi_t(i,j) ecost[i,j] from the
node and edge marginals m = d logZ / d em, sum_t xi_t = d logZ / d trans_b taken with create_graph (which is d/d lambda of
logZ(em + lambda cost, trans + lambda ecost) at 0 written out); every gradient comes from a second autograd.grad through it.  With
the costs leaves it is the oracle of the C ABI; with the costs built from the parameters themselves it is the oracle of the
entropy (H = logZ - E_p[score]) and of KL(p || q).  test_crf_path.py pins all of it against enumeration of all paths.

Error model: ``centred`` below, crf_risk_cases.centred extended with the edge terms (F = E o ecost in the forward mean, in eq /
dq of the backward, N = sum_t outer(abar_{t-1}, ui_t) beside G), run in float32; run in float64 it agrees with the reference to
1e-9 of max(1, max|ref|) (test_crf_path.py).

Acceptance rule: |got - ref64| <= max(T_proj, 4 max|centred32 - ref64|), T_proj = 2e-5 max|ref| for risk and logz, 1e-4 max|ref|
+ 1e-7 for every gradient (decost like dtrans; the z* quantities are the gradients of sum_b w[b] logZ[b], what gz produces).
Entropy and KL are differences of large terms: for their values T_proj = 2e-5 max|logZ|, the pllh provision of
crf_lattice_cases.  Against a vacuous bound every bound is asserted to be at most 1e-3 max|ref64| + 1e-7 (entropy / KL values:
1e-3 max|logZ| + 1e-7)."""
import functools
import types

import torch

import crf_lattice_cases as X
import crf_llh_cases as L
import crf_risk_cases as R

SHAPES = R.SHAPES
BRUTE = R.BRUTE
# cost patterns: (b) randn node plus randn edge, (e) edge only, (c) node only, (s) the chain's own score (entropy), (z) zeros,
# (n) (b) with NaN at the masked columns of the node cost
PATTERNS = ("b", "e", "c", "s", "z", "n")
GRADS = ("dem", "dstart", "dend", "dtrans", "dcost", "decost")
ZGRADS = ("zem", "zstart", "zend", "ztrans")
QUANTITIES = ("risk", "logz") + GRADS + ZGRADS
live = R.live


def score_cost(inp):
    """The chain's own score as a path cost: node = emissions + start at column 0 + end at the last live column, edge = trans."""
    em, _, mask, start, end, trans = inp
    cost = em.clone()
    cost[:, 0] += start
    cost[torch.arange(em.shape[0]), X.lengths_of(mask) - 1] += end
    return cost * live(mask)[..., None], trans.clone()


def make_costs(shape, pattern, inp):
    """-> (cost [B,S,C] or None, ecost [C,C] or None) of a pattern."""
    em = inp[0]
    C = em.shape[2]
    node = R.make_cost(shape, "n" if pattern == "n" else "r", inp)
    edge = torch.randn(C, C, generator=torch.Generator().manual_seed(91 + sum(shape)))
    if pattern in ("b", "n"):
        return node, edge
    if pattern == "e":
        return None, edge
    if pattern == "c":
        return node, None
    if pattern == "s":
        return score_cost(inp)
    if pattern == "z":
        return torch.zeros_like(em), torch.zeros(C, C)
    raise ValueError(pattern)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def log_partition(em, mask, start, end, trans_b):
    """crf_lattice_cases.log_partition without sets and with one transition matrix per sentence, trans_b [B,C,C]."""
    score = start[None] + em[:, 0]
    for t in range(1, em.shape[1]):
        nxt = torch.logsumexp(score[:, :, None] + trans_b, dim=1) + em[:, t]
        score = torch.where(mask[:, t, None].bool(), nxt, score)
    return torch.logsumexp(score + end[None], dim=1)


def expect(em_, s_, e_, t_, mask, cost, ecost):
    """-> (R [B], logZ [B], node marginals [B,S,C], summed edge marginals [B,C,C]), all differentiable: the expectation under
    the chain (em_, s_, e_, t_) of the path cost (cost [B,S,C], ecost [C,C]; tensors that may themselves depend on parameters)."""
    B, S, C = em_.shape
    on = live(mask)[..., None]
    tb = t_.unsqueeze(0).expand(B, C, C)
    logz = log_partition(em_, mask, s_, e_, tb)
    m, xi = torch.autograd.grad(logz.sum(), [em_, tb], create_graph=True, allow_unused=True)  # (S = 1: no transition)
    xi = torch.zeros_like(tb) if xi is None else xi
    m = m * on
    risk = (m * torch.where(on, cost, torch.zeros((), dtype=cost.dtype))).sum((1, 2)) + (xi * ecost[None]).sum((1, 2))
    return risk, logz, m, xi


def _leaves(inp, dtype):
    em, _, mask, start, end, trans = inp
    return tuple(x.to(dtype).clone().requires_grad_(True) for x in (em, start, end, trans))


def _grads(obj, params):
    g = torch.autograd.grad(obj, params, allow_unused=True, retain_graph=True)
    return [torch.zeros_like(p) if x is None else x.detach() for x, p in zip(g, params)]


def oracle(inp, cost, ecost, w, dtype=torch.float64):
    """Every quantity of the C ABI: risk, logz, the gradients of sum_b w[b] R[b] (d*) and of sum_b w[b] logZ[b] (z*)."""
    mask = inp[2]
    B, S, C = inp[0].shape
    on = live(mask)[..., None]
    em_, s_, e_, t_ = _leaves(inp, dtype)
    zero = torch.zeros((), dtype=dtype)
    c_ = (torch.zeros(B, S, C, dtype=dtype) if cost is None else torch.where(on, cost.to(dtype), zero)).requires_grad_(True)
    ec_ = (torch.zeros(C, C, dtype=dtype) if ecost is None else ecost.to(dtype).clone()).requires_grad_(True)
    risk, logz, _, _ = expect(em_, s_, e_, t_, mask, c_, ec_)
    wd = w.to(dtype)
    dem, dstart, dend, dtrans, dcost, decost = _grads((risk * wd).sum(), [em_, s_, e_, t_, c_, ec_])
    zem, zstart, zend, ztrans = _grads((logz * wd).sum(), [em_, s_, e_, t_])
    return dict(risk=risk.detach(), logz=logz.detach(), dem=dem * on, dstart=dstart, dend=dend, dtrans=dtrans, dcost=dcost * on,
                decost=decost, zem=zem * on, zstart=zstart, zend=zend, ztrans=ztrans)


def _score_parts(em_, s_, e_, t_, mask):
    B = em_.shape[0]
    first = torch.zeros_like(em_)
    first[:, 0] = 1.0
    last = torch.zeros_like(em_)
    last[torch.arange(B), X.lengths_of(mask) - 1] = 1.0
    return em_ + first * s_[None, None] + last * e_[None, None], t_


def entropy_oracle(inp, w, dtype=torch.float64):
    """H [B] = logZ - E_p[score] and the gradients of sum_b w[b] H[b], by autograd through the score's own dependence on the
    parameters."""
    mask = inp[2]
    on = live(mask)[..., None]
    em_, s_, e_, t_ = _leaves(inp, dtype)
    cost, ecost = _score_parts(em_, s_, e_, t_, mask)
    risk, logz, _, _ = expect(em_, s_, e_, t_, mask, cost, ecost)
    h = logz - risk
    dem, dstart, dend, dtrans = _grads((h * w.to(dtype)).sum(), [em_, s_, e_, t_])
    return dict(h=h.detach(), logz=logz.detach(), dem=dem * on, dstart=dstart, dend=dend, dtrans=dtrans)


def kl_oracle(inp_p, inp_q, w, shared=False, dtype=torch.float64):
    """KL(p || q) [B] and the gradients of sum_b w[b] KL[b] to both sides (``shared``: q's parameters are p's, and their
    gradients hold both contributions)."""
    mask = inp_p[2]
    on = live(mask)[..., None]
    pe, ps, pend, pt = _leaves(inp_p, dtype)
    qe, qs, qend, qt = _leaves(inp_q, dtype)
    if shared:
        qs, qend, qt = ps, pend, pt
    cp, ecp = _score_parts(pe, ps, pend, pt, mask)
    cq, ecq = _score_parts(qe, qs, qend, qt, mask)
    risk, logz_p, _, _ = expect(pe, ps, pend, pt, mask, cp - cq, ecp - ecq)
    logz_q = log_partition(qe, mask, qs, qend, qt.unsqueeze(0).expand(pe.shape[0], -1, -1))
    kl = risk - logz_p + logz_q
    obj = (kl * w.to(dtype)).sum()
    dem_p, dstart_p, dend_p, dtrans_p = _grads(obj, [pe, ps, pend, pt])
    out = dict(kl=kl.detach(), logz=torch.maximum(logz_p.detach().abs(), logz_q.detach().abs()), dem_p=dem_p * on,
               dstart_p=dstart_p, dend_p=dend_p, dtrans_p=dtrans_p)
    out["dem_q"] = _grads(obj, [qe])[0] * on
    if not shared:
        out["dstart_q"], out["dend_q"], out["dtrans_q"] = _grads(obj, [qs, qend, qt])
    return out


# ---- the centred recursions --------------------------------------------------------------------------------------------------
def centred(inp, cost, ecost, w, dtype=torch.float32):
    """Every quantity of ``oracle`` by the centred recursions with the edge terms, sentence by sentence, in ``dtype``."""
    em, _, mask, start, end, trans = (x if x.dtype in (torch.uint8, torch.int64, torch.bool) else x.to(dtype) for x in inp)
    B, S, C = em.shape
    cost = torch.zeros(B, S, C, dtype=dtype) if cost is None else cost.to(dtype)
    ecost = torch.zeros(C, C, dtype=dtype) if ecost is None else ecost.to(dtype)
    w = w.to(dtype)
    lens = X.lengths_of(mask)
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    out = dict(risk=z(B), logz=z(B), dem=z(B, S, C), dcost=z(B, S, C), dstart=z(C), dend=z(C), dtrans=z(C, C), decost=z(C, C),
               zem=z(B, S, C), zstart=z(C), zend=z(C), ztrans=z(C, C))
    tmax = trans.max()
    E = torch.exp(trans - tmax)
    F = E * ecost
    for b in range(B):
        n = int(lens[b])
        e, c = em[b, :n], cost[b, :n]
        mx = e.max(1).values
        abar, sp, ac, mean = [None] * n, [None] * n, [None] * n, [None] * n
        a0 = start + e[0]
        s = torch.exp(a0 - a0.max())
        lz = a0.max() + torch.log(s.sum())
        abar[0] = s / s.sum()
        at = c[0]
        for t in range(n):
            if t >= 1:
                sp[t] = abar[t - 1] @ E
                at = c[t] + ((abar[t - 1] * ac[t - 1]) @ E + abar[t - 1] @ F) / sp[t]
                s = sp[t] * torch.exp(e[t] - mx[t])
                lz = lz + tmax + mx[t] + torch.log(s.sum())
                abar[t] = s / s.sum()
            mean[t] = (abar[t] * at).sum()
            ac[t] = at - mean[t]
        pe = abar[n - 1] * torch.exp(end - end.max())
        out["logz"][b] = lz + end.max() + torch.log(pe.sum())
        pe = pe / pe.sum()
        out["risk"][b] = (torch.stack(mean).double().sum() + (pe * ac[n - 1]).sum().double()).to(dtype)
        bt, bh = torch.exp(end - end.max()), z(C)
        G, N = z(C, C), z(C, C)
        val, marg = [None] * n, [None] * n
        for t in range(n - 1, 0, -1):
            u = torch.exp(e[t] - mx[t]) * bt
            d = (sp[t] * u).sum()
            ui = u / d
            mu = sp[t] * ui
            q = u * (c[t] + bh)
            eu, eq = E @ u, E @ q + F @ u
            dq = (abar[t - 1] * eq).sum()
            dv = ac[t] + bh
            dbar = (mu * dv).sum()
            val[t], marg[t] = mu * (dv - dbar), mu
            k = ui * (c[t] + bh - dbar - mean[t])
            G = G + torch.outer(abar[t - 1] * ac[t - 1], ui) + torch.outer(abar[t - 1], k)
            N = N + torch.outer(abar[t - 1], ui)
            bt, bh = eu / d, eq / eu - dq / d
        p0 = abar[0] * bt
        p0 = p0 / p0.sum()
        dv = ac[0] + bh
        val[0], marg[0] = p0 * (dv - (p0 * dv).sum()), p0
        val, marg = torch.stack(val), torch.stack(marg)
        out["dem"][b, :n] = w[b] * val
        out["dcost"][b, :n] = w[b] * marg
        out["zem"][b, :n] = w[b] * marg
        out["dstart"] += w[b] * val[0]
        out["dend"] += w[b] * val[n - 1]
        out["zstart"] += w[b] * marg[0]
        out["zend"] += w[b] * marg[n - 1]
        out["dtrans"] += w[b] * (G * E + N * F)
        out["decost"] += w[b] * N * E
        out["ztrans"] += w[b] * N * E
    return out


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def bound(name, r64, c32, scale=None):
    """The acceptance bound of one quantity; ``scale``: max|logZ| for a value that is a difference of large terms."""
    m = float(r64.abs().max())
    if scale is not None:
        t_proj, cap = 2e-5 * scale, 1e-3 * scale + 1e-7
    elif name in ("risk", "logz"):
        t_proj, cap = 2e-5 * m, 1e-3 * m + 1e-7
    else:
        t_proj, cap = 1e-4 * m + 1e-7, 1e-3 * m + 1e-7
    bnd = max(t_proj, 4.0 * float((c32.double() - r64).abs().max()))
    assert bnd <= cap, f"vacuous bound for {name}: {bnd:.3e} > {cap:.3e}"  # (an error model gone wrong would accept anything)
    return bnd


def make_reference(inp, cost, ecost, w=None):
    w = L.weights(inp[0].shape[0]) if w is None else w
    r64, c32 = oracle(inp, cost, ecost, w), centred(inp, cost, ecost, w)
    return types.SimpleNamespace(inputs=inp, cost=cost, ecost=ecost, w=w, r64=r64, c32=c32,
                                 bound={k: bound(k, r64[k], c32[k]) for k in QUANTITIES})


@functools.lru_cache(maxsize=None)
def reference(shape, pattern):
    """Inputs, costs, float64 reference, centred float32 restatement and bounds of one case: computed once, shared, not to be
    modified.  Patterns (z) and (n) have no reference of their own (exact zeros; (b)'s bits)."""
    assert pattern in ("b", "e", "c", "s")
    inp = X.inputs(shape)
    return make_reference(inp, *make_costs(shape, pattern, inp))


@functools.lru_cache(maxsize=None)
def entropy_reference(shape):
    """The entropy and its gradients in float64 by autograd; the error model is (s)'s centred float32 run: H = logz - risk in
    float32 and the cost-covariance gradients negated."""
    ref = reference(shape, "s")
    r64 = entropy_oracle(ref.inputs, ref.w)
    c32 = dict(h=ref.c32["logz"] - ref.c32["risk"], **{k: -ref.c32[k] for k in ("dem", "dstart", "dend", "dtrans")})
    scale = float(r64["logz"].abs().max())
    bnd = {k: bound(k, r64[k], c32[k], scale if k == "h" else None) for k in c32}
    return types.SimpleNamespace(inputs=ref.inputs, w=ref.w, r64=r64, c32=c32, bound=bnd)


def kl_inputs(shape, shared):
    """p = crf_lattice_cases.inputs; q = other emissions on the same mask and (unless ``shared``) other parameters."""
    p = X.inputs(shape)
    g = torch.Generator().manual_seed(67 + sum(shape))
    sc = float(shape[3])
    eq = p[0] + 0.5 * sc * torch.randn(p[0].shape, generator=g)
    if shared:
        return p, (eq,) + tuple(p[1:])
    jit = lambda x, s: x + s * torch.randn(x.shape, generator=g)
    return p, (eq, p[1], p[2], jit(p[3], 0.3), jit(p[4], 0.3), jit(p[5], 0.3 * sc))


@functools.lru_cache(maxsize=None)
def kl_reference(shape, shared):
    inp_p, inp_q = kl_inputs(shape, shared)
    w = L.weights(shape[0])
    r64 = kl_oracle(inp_p, inp_q, w, shared)
    # error model: the engine's composition, from centred float32 runs on p (score difference as cost) and on q (no cost)
    f32 = lambda inp: tuple(x if x.dtype in (torch.uint8, torch.int64, torch.bool) else x.float() for x in inp)
    cp, ecp = score_cost(f32(inp_p))
    cq, ecq = score_cost(f32(inp_q))
    P = centred(inp_p, cp - cq, ecp - ecq, w)
    Q = centred(inp_q, None, None, w)
    last = X.lengths_of(inp_p[2]) - 1
    rows = torch.arange(shape[0])
    c32 = dict(kl=(P["risk"] - P["logz"]) + Q["logz"], dem_p=P["dem"], dstart_p=P["dstart"], dend_p=P["dend"], dtrans_p=P["dtrans"],
               dem_q=Q["zem"] - P["dcost"])
    q_par = dict(dstart_q=Q["zstart"] - P["dcost"][:, 0].sum(0), dend_q=Q["zend"] - P["dcost"][rows, last].sum(0),
                 dtrans_q=Q["ztrans"] - P["decost"])
    if shared:
        for k, v in q_par.items():
            c32[k[:-1] + "p"] = c32[k[:-1] + "p"] + v
    else:
        c32.update(q_par)
    scale = float(r64["logz"].max())
    bnd = {k: bound(k, r64[k], c32[k], scale if k == "kl" else None) for k in c32}
    return types.SimpleNamespace(p=inp_p, q=inp_q, w=w, r64=r64, c32=c32, bound=bnd)


WORST = {}


def check(ref, name, got, add=None, tag=None):
    """Assert ``got`` against the float64 reference (plus ``add``, for accumulated gradients); prints err / bound."""
    r64 = ref.r64[name] if add is None else ref.r64[name] + add
    bnd = ref.bound[name]
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    err = float((got - r64).abs().max())
    r = err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf"))  # (a reference that is identically 0, met exactly)
    key = tag or name
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"crf-path ratio {key} {r:.4f} (err {err:.3e}, bound {bnd:.3e}; worst so far {WORST[key]:.4f})")
    assert r <= 1.0, f"{name}: err / bound = {r:.3f}"


def bruteforce(inp, cost, ecost, w, inp_q=None):
    """By enumerating all C^L paths in float64: risk [B], entropy [B], KL(p || q) [B] (``inp_q`` given, else None), and dem
    [B,S,C], dtrans [C,C], decost [C,C] of sum_b w[b] R[b]:  dR/dtheta = sum_y p(y) f_theta(y) (W(y) - R), decost[i,j] = sum_y
    p(y) #{t: y_{t-1} = i, y_t = j}."""
    em, _, mask, start, end, trans = inp
    B, S, C = em.shape
    cd = torch.zeros(B, S, C, dtype=torch.float64) if cost is None else cost.double()
    ed = torch.zeros(C, C, dtype=torch.float64) if ecost is None else ecost.double()
    wd = w.double()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    risk, ent, kl, dem, dtrans, decost = z(B), z(B), z(B), z(B, S, C), z(C, C), z(C, C)

    def scores(inp_, b, paths, n):
        e_, _, _, s_, en_, t_ = (x.double() if x.is_floating_point() else x for x in inp_)
        sc = s_[paths[:, 0]] + e_[b, 0, paths[:, 0]] + en_[paths[:, -1]]
        for t in range(1, n):
            sc = sc + t_[paths[:, t - 1], paths[:, t]] + e_[b, t, paths[:, t]]
        return sc - torch.logsumexp(sc, 0)

    for b in range(B):
        n = int(X.lengths_of(mask)[b])
        paths = torch.cartesian_prod(*[torch.arange(C)] * n).reshape(-1, n)
        logp = scores(inp, b, paths, n)
        p = torch.exp(logp)
        wy = cd[b, 0, paths[:, 0]]
        for t in range(1, n):
            wy = wy + cd[b, t, paths[:, t]] + ed[paths[:, t - 1], paths[:, t]]
        risk[b] = (p * wy).sum()
        ent[b] = -(p * logp).sum()
        if inp_q is not None:
            kl[b] = (p * (logp - scores(inp_q, b, paths, n))).sum()
        dev = p * (wy - risk[b])
        for t in range(n):
            dem[b, t].index_add_(0, paths[:, t], wd[b] * dev)
            if t >= 1:
                dtrans.view(-1).index_add_(0, paths[:, t - 1] * C + paths[:, t], wd[b] * dev)
                decost.view(-1).index_add_(0, paths[:, t - 1] * C + paths[:, t], wd[b] * p)
    return dict(risk=risk, entropy=ent, kl=kl if inp_q is not None else None, dem=dem, dtrans=dtrans, decost=decost)
