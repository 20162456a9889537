"""Case table and float64 restatement of the token-level divergence kernels (include/mtvaf_hip.h: mtvaf_token_divergence_fwd / _bwd;
DESIGN.md section 4.27), shared by test_token_div.py (CPU: proves the restatement) and test_token_div_gpu.py.  The restatement is
the definition with plain ``log_softmax`` in float64 -- not the kernel's arithmetic."""
import functools
import math

import torch

KINDS = ("sym_kl", "js")
REDUCTIONS = ("token_mean", "batch_mean")
# (N, C): one tag, two, the tagger's 11, both sides of the layout switch (16 | 17), the widest rows, rows that are no multiple
# of the rows of a wave (4 | 1) or of a block (16 | 4), more than one block, and the headline shape
SHAPES = [(1, 1), (1, 2), (3, 11), (5, 16), (5, 17), (7, 63), (2, 64), (65, 11), (257, 11), (4096, 11)]
MASKS = ("none", "prefix", "one", "dead")
TEMPERATURES = (1.0, 0.5, 3.0)
UPSTREAM = 1.7   # factor in front of the loss when the gradients are taken
BATCH = {1: 1, 3: 3, 5: 5, 7: 7, 2: 2, 65: 5, 257: 1, 4096: 32}  # B of the batch mean for every N (N = B * S where B | N)


def make_logits(N, C, s=3.0, d=1.0, seed=None):
    """-> x, y fp32 [N,C]:  x = s * randn,  y = x + d * s * randn"""
    g = torch.Generator().manual_seed(100 * N + C if seed is None else seed)
    x = s * torch.randn(N, C, generator=g)
    return x, x + d * s * torch.randn(N, C, generator=g)


def make_mask(name, N):
    """-> uint8 [N] or None.  "prefix": ragged prefix lengths over sentences of 8 rows (one sentence of N rows below 8)."""
    if name == "none":
        return None
    m = torch.zeros(N, dtype=torch.uint8)
    if name == "prefix":
        S = 8 if N >= 8 else N
        for b, start in enumerate(range(0, N, S)):
            n = min(S, N - start)
            m[start:start + (max(1, (3 * b + 5) % n) if n > 1 else 1)] = 1   # 1 .. n - 1 live rows: every sentence has a dead one
    elif name == "one":
        m[N // 2] = 1
    elif name != "dead":
        raise ValueError(name)
    return m


def row_values(x, y, kind, temperature=1.0):
    """[N] float64 (or the dtype of x when it is float64 already): every row's divergence, masked or not"""
    lp = torch.log_softmax(x.double() / temperature, -1)
    lq = torch.log_softmax(y.double() / temperature, -1)
    p, q = lp.exp(), lq.exp()
    if kind == "sym_kl":
        return 0.5 * ((p - q) * (lp - lq)).sum(-1)
    if kind == "js":
        lm = torch.logaddexp(lp, lq) - math.log(2.0)
        return 0.5 * (p * (lp - lm)).sum(-1) + 0.5 * (q * (lq - lm)).sum(-1)
    raise ValueError(kind)


def token_div_ref(x, y, mask, kind, temperature=1.0, reduction="token_mean", B=1, scale=1.0):
    """-> (loss 0-dim float64, rows [N] float64 with 0 on masked rows).  Masked rows are replaced before anything is computed,
    so whatever they hold (NaN, inf) reaches neither the value nor a gradient."""
    live = torch.ones(x.shape[0], dtype=torch.bool) if mask is None else mask != 0
    xs = torch.where(live[:, None], x.double(), torch.zeros((), dtype=torch.float64))
    ys = torch.where(live[:, None], y.double(), torch.zeros((), dtype=torch.float64))
    rows = row_values(xs, ys, kind, temperature) * live
    D = int(live.sum()) if reduction == "token_mean" else B
    loss = scale * rows.sum() / D if D > 0 else rows.sum() * 0.0
    return loss, rows


def ref_with_grads(x, y, mask, kind, temperature=1.0, reduction="token_mean", B=1, scale=1.0):
    """-> (loss, rows, d(UPSTREAM * loss)/dx, d(UPSTREAM * loss)/dy), all float64, by autograd"""
    xd, yd = x.double().clone().requires_grad_(True), y.double().clone().requires_grad_(True)
    loss, rows = token_div_ref(xd, yd, mask, kind, temperature, reduction, B, scale)
    gx, gy = torch.autograd.grad(UPSTREAM * loss, (xd, yd))
    return loss.detach(), rows.detach(), gx, gy


@functools.lru_cache(maxsize=None)
def reference(shape, mask_name, kind, temperature, reduction):
    """One case: computed once, shared, not to be modified.  -> (x, y, mask, loss, rows, gx, gy)"""
    x, y = make_logits(*shape)
    mask = make_mask(mask_name, shape[0])
    return (x, y, mask) + ref_with_grads(x, y, mask, kind, temperature, reduction, BATCH[shape[0]])


def extreme_logits(N=6, C=11, big=1e4):
    """Rows +-big * one-hot with the two passes on different tags: both distributions are point masses apart from each other.
    The last row has both passes on the same tag."""
    x, y = torch.zeros(N, C), torch.zeros(N, C)
    for r in range(N):
        sign = 1.0 if r % 2 == 0 else -1.0
        x[r, r % C] = sign * big
        y[r, (r + 1) % C if r < N - 1 else r % C] = sign * big
    return x, y


# ---- the identity of CRF.symmetric_kl, by enumeration -----------------------------------------------------------------------
def chain_sym_kl_bruteforce(em_a, em_b, start, end, trans, lengths):
    """-> (KL(a||b) + KL(b||a) [B], E_a[D] - E_b[D] [B]) in float64 over every path of every sentence, D = em_a - em_b; both
    chains share start / end / trans."""
    import itertools
    B, S, C = em_a.shape
    kl, ident = [], []
    for b in range(B):
        n = int(lengths[b])
        paths = list(itertools.product(range(C), repeat=n))

        def scores(em):
            out = []
            for path in paths:
                s = start[path[0]] + end[path[-1]] + sum(em[b, t, path[t]] for t in range(n))
                s = s + sum(trans[path[t - 1], path[t]] for t in range(1, n))
                out.append(s)
            return torch.log_softmax(torch.stack(out), 0)

        la, lb = scores(em_a), scores(em_b)
        pa, pb = la.exp(), lb.exp()
        kl.append((pa * (la - lb)).sum() + (pb * (lb - la)).sum())
        delta = torch.stack([sum((em_a - em_b)[b, t, path[t]] for t in range(n)) for path in paths])
        ident.append((pa * delta).sum() - (pb * delta).sum())
    return torch.stack(kl), torch.stack(ident)
