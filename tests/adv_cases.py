"""Case table, input builders, the plain float64 restatement of the contract of mtvaf_adv_perturb (include/mtvaf_hip.h,
csrc/adversarial.hip) and the bound its fp32 arithmetic is held to.  Shared by test_adv_cases.py (CPU: proves the restatement) and
test_adv_gpu.py (the kernel, the embedding tap, Adversary).  Nothing here imports mtvaf_amd: torch on the host, float64 from the fp32
inputs.

The bound, derived from the arithmetic the kernel uses (u = 2^-24, one fp32 rounding; nothing below is fitted to an output):

  * every sum of squares is formed in double from the first operation: its error (n 2^-53 relative) vanishes beside the ONE rounding
    of the norm to fp32, so a norm is off by <= u relative (stats: 2 u allowed).
  * L2 without delta_in (FGM): delta = eps * (g / n32).  n32 carries u, the division u, the product u: 3 u |ref| to first order;
    held to 4 u |ref|.
  * Linf without delta_in: eps * (+-1 or 0) is exact: 0.
  * Linf with delta_in: delta_in + step * sign(g) is one rounded addition (or one fused multiply-add), the clamp is exact:
    u (|delta_in| + step).
  * L2 with delta_in: t = step * (g / n32) carries 3 u |t|, the addition u |d|: with A = |delta_in| + |t| >= |d| elementwise,
    e_d <= 4 u A.  The unit norm of the rounded d is off by at most |e_d|_u <= 4 u |A|_u, and by u from its rounding to fp32:
    relative r <= 4 u |A|_u / |d|_u + u.  Projected, out = d * (eps / n32): the quotient u, the product u, so
    |out - ref| <= c e_d + |ref| (r + 2 u) with c = min(1, eps / |d|_u) <= 1;  held to  4 u A + |ref| (4 u |A|_u / |d|_u + 3 u).
    A unit the reference projects and the kernel does not (or the reverse) sits within r of the sphere: the two results differ by
    e_d + |d| r, inside the same expression -- it is applied to every unit, projected or not.
  * a degenerate unit (|g|_u 0, inf or NaN after rounding to fp32) has t = 0 exactly: the same expressions with A = |delta_in|.
  * stats[:,1] is the double norm of the kernel's OWN delta_out rounded once: off from the reference's by at most the L2 norm of
    the element bounds over the sentence, plus 2 u |ref|.
Second-order terms (u^2) are covered by the one u of head-room each count above carries."""
import torch

U32 = 2.0 ** -24
NORMS = ("l2", "linf")
SCOPES = ("sentence", "token")
DELTA_MODES = (None, "bites", "inside")  # no delta_in (FGM) / a delta_in the projection cuts back / one it leaves alone
EPS, STEP = 0.5, 0.125                   # (exact in fp32)


def _case(cid, B, S, H, mask="ragged"):
    return dict(id=cid, B=B, S=S, H=H, mask=mask)


CASES = [
    _case("B1-S1-H1-smallest", 1, 1, 1, mask="full"),
    _case("B2-S3-H5-scalar-tail-only", 2, 3, 5),
    _case("B3-S16-H128-lengths-16-6-0-dead-sentence", 3, 16, 128, mask=[16, 6, 0]),
    _case("B2-S65-H3-every-other-row", 2, 65, 3, mask="alternate"),
    _case("B2-S7-H768-real-row", 2, 7, 768),
    _case("B33-S5-H64-more-sentences-than-a-small-grid", 33, 5, 64),
    _case("B1-S512-H1024-the-limit", 1, 512, 1024, mask="full"),
]


def make_mask(case):
    B, S, kind = case["B"], case["S"], case["mask"]
    m = torch.zeros(B, S, dtype=torch.uint8)
    if kind == "full":
        m[:] = 1
    elif kind == "alternate":
        m[:, ::2] = 1
        m[1] = 1 - m[1]  # (the second sentence keeps the odd rows)
    else:
        lengths = kind if isinstance(kind, list) else [max(1, S - (3 * b) % S) for b in range(B)]
        for b, n in enumerate(lengths):
            m[b, :n] = 1
    return m


def make_inputs(case, delta_mode=None, seed=0):
    """-> g [B,S,H] fp32, mask [B,S] u8, delta_in or None.  "bites": |delta_in|_u is around sqrt(elements) * eps, far outside the
    ball for all but the one- and few-element units; "inside": 1e-4 eps per element, |delta_in|_u + step < eps for every unit up to
    the limit shape (sqrt(512 * 1024) * 1e-4 = 0.07)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    B, S, H = case["B"], case["S"], case["H"]
    g = torch.randn(B, S, H, generator=gen) * 1e-3
    delta = None
    if delta_mode is not None:
        delta = torch.randn(B, S, H, generator=gen) * (EPS if delta_mode == "bites" else 1e-4 * EPS)
    return g, make_mask(case), delta


def fits32(n):
    """a norm that fp32 holds and that is not 0: the unit takes its gradient term"""
    n32 = n.to(torch.float32)
    return torch.isfinite(n32) & (n32 > 0)


def unit_norm(v, scope):
    """v [B,S,H] float64, dead rows zero -> [B,S,1]: the L2 norm of the unit every row belongs to"""
    sq = (v * v).sum(-1)
    if scope == "sentence":
        sq = sq.sum(1, keepdim=True).expand_as(sq)
    return sq.sqrt()[..., None]


def reference(g, mask, eps, step=0.0, norm="l2", scope="sentence", delta_in=None):
    """The contract in float64 -> dict: delta [B,S,H], stats [B,2] (gradient norm over the live rows -- inf / NaN where the
    gradient holds one --, norm of delta), tol [B,S,H] and stats_tol [B,2]: the bounds of the module docstring."""
    live = mask.ne(0)[..., None]
    zero = torch.zeros((), dtype=torch.float64)
    g64 = torch.where(live, g.double(), zero)
    ng = unit_norm(g64, scope)
    ok = fits32(ng)
    gs = torch.where(ok, g64, zero)
    t = gs / torch.where(ok, ng, zero + 1) if norm == "l2" else torch.sign(gs)
    if delta_in is None:
        d = eps * t
        tol = 4 * U32 * d.abs() if norm == "l2" else torch.zeros_like(d)
    else:
        din = torch.where(live, delta_in.double(), zero)
        d = din + step * t
        A = din.abs() + (step * t).abs()
        if norm == "linf":
            d = d.clamp(-eps, eps)
            tol = U32 * (din.abs() + step)
        else:
            nd = unit_norm(d, scope)
            d = torch.where(nd > eps, d * (eps / nd.clamp_min(1e-300)), d)
            rel = 4 * U32 * unit_norm(A, scope) / nd.clamp_min(1e-300) + 3 * U32
            tol = 4 * U32 * A + d.abs() * torch.where(nd > 0, rel, zero)
    d = torch.where(live, d, zero)
    tol = torch.where(live, tol, zero)
    gnorm = (g64 * g64).sum((1, 2)).sqrt()
    dnorm = (d * d).sum((1, 2)).sqrt()
    stats = torch.stack([gnorm, dnorm], 1)
    stats_tol = torch.stack([2 * U32 * gnorm, (tol * tol).sum((1, 2)).sqrt() + 2 * U32 * dnorm], 1)
    return dict(delta=d, stats=stats, tol=tol, stats_tol=stats_tol)


def excess(got, ref, tol):
    """max |got - ref| / tol over the elements (0 where both the error and the bound are 0; inf where got is not finite)"""
    got, ref = got.detach().double().cpu(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    return float(q.max()) if q.numel() else 0.0
