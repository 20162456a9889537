"""Case table and float64 restatement of the token cross-entropy kernels (include/mtvaf_hip.h: mtvaf_token_ce_fwd / _bwd /
mtvaf_token_argmax), shared by test_token_ce.py (CPU: proves the restatement against torch) and the GPU
tests.  The restatement is the definition with plain ``log_softmax`` in float64 -- not the kernel's arithmetic."""
import functools

import torch

REDUCTIONS = ("mean", "batch_mean", "sum")
# (N, C): one tag, two, the tagger's 11, both sides of the lane-group switch (16 | 17), the widest rows, rows that do not fill a
# wave (4 | 1 rows) or a block (16 | 4), more than one block, more than one pass of the finishing block (1025), the headline shape
SHAPES = [(1, 1), (1, 2), (3, 11), (5, 16), (5, 17), (7, 63), (2, 64), (65, 11), (257, 11), (1025, 11), (4096, 11)]
MASKS = ("none", "prefix", "one", "dead")
SMOOTHINGS = (0.0, 0.1)
GAMMAS = (0.0, 1.0, 2.0, 3.5)
IGNORE = -100
UPSTREAM = 1.7   # factor in front of the loss when the gradients are taken
BATCH = {1: 1, 3: 3, 5: 5, 7: 7, 2: 2, 65: 5, 257: 1, 1025: 25, 4096: 32}  # B of the batch mean for every N


def make_logits(N, C, s=3.0, seed=None):
    g = torch.Generator().manual_seed(100 * N + C if seed is None else seed)
    return s * torch.randn(N, C, generator=g)


def make_labels(N, C, seed=None):
    """Uniform labels, every fifth row (4, 9, ...) at IGNORE."""
    g = torch.Generator().manual_seed(7 + 100 * N + C if seed is None else seed)
    y = torch.randint(0, C, (N,), generator=g)
    y[4::5] = IGNORE
    return y


def make_weights(C, seed=None):
    """Random class weights in [0.1, 1.1] with one weight at 0."""
    g = torch.Generator().manual_seed(13 + C if seed is None else seed)
    w = 0.1 + torch.rand(C, generator=g)
    w[C // 2] = 0.0
    return w


def make_mask(name, N):
    """-> uint8 [N] or None.  "prefix": ragged prefix lengths over sentences of 8 rows (one sentence of N rows below 8)."""
    if name == "none":
        return None
    m = torch.zeros(N, dtype=torch.uint8)
    if name == "prefix":
        S = 8 if N >= 8 else N
        for b, start in enumerate(range(0, N, S)):
            n = min(S, N - start)
            m[start:start + (max(1, (3 * b + 5) % n) if n > 1 else 1)] = 1
    elif name == "one":
        m[N // 2] = 1
    elif name != "dead":
        raise ValueError(name)
    return m


def live_rows(labels, mask, C, ignore_index=IGNORE):
    live = (labels != ignore_index) & (labels >= 0) & (labels < C)
    return live if mask is None else live & (mask != 0)


def row_values(z, labels, live, weight=None, smoothing=0.0, gamma=0.0):
    """[N] float64: every row's L, 0 on dead rows (which are replaced before anything is computed).  ``z`` float64 [N,C]."""
    N, C = z.shape
    zs = torch.where(live[:, None], z, torch.zeros((), dtype=torch.float64))
    y = torch.where(live, labels, torch.zeros_like(labels))
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    lp = torch.log_softmax(zs, -1)
    onehot = torch.nn.functional.one_hot(y, C).double()
    a = (1.0 - smoothing) * w[y][:, None] * onehot + (smoothing / C) * w[None, :]
    ce = -(a * lp).sum(-1)
    if gamma == 0.0:
        L = ce
    else:
        om = (lp.exp() * (1.0 - onehot)).sum(-1)
        L = om.pow(gamma) * ce
    return L * live


def token_ce_ref(z, labels, mask=None, weight=None, smoothing=0.0, gamma=0.0, reduction="mean", B=1, scale=1.0, ignore_index=IGNORE):
    """-> (loss 0-dim float64, rows [N] float64).  ``z`` float64 [N,C]."""
    C = z.shape[1]
    live = live_rows(labels, mask, C, ignore_index)
    rows = row_values(z, labels, live, weight, smoothing, gamma)
    if reduction == "mean":
        w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
        D = float((w[torch.where(live, labels, torch.zeros_like(labels))] * live).sum())
    else:
        D = float(B) if reduction == "batch_mean" else 1.0
    loss = scale * rows.sum() / D if D > 0 else rows.sum() * 0.0
    return loss, rows


def formula_grad(z, labels, live, weight=None, smoothing=0.0, gamma=0.0):
    """The documented dL/dz [N,C] in float64, zeros on dead rows."""
    N, C = z.shape
    zs = torch.where(live[:, None], z, torch.zeros((), dtype=torch.float64))
    y = torch.where(live, labels, torch.zeros_like(labels))
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    lp = torch.log_softmax(zs, -1)
    p = lp.exp()
    onehot = torch.nn.functional.one_hot(y, C).double()
    a = (1.0 - smoothing) * w[y][:, None] * onehot + (smoothing / C) * w[None, :]
    A = a.sum(-1, keepdim=True)
    ce = -(a * lp).sum(-1, keepdim=True)
    if gamma == 0.0:
        g = A * p - a
    else:
        om = (p * (1.0 - onehot)).sum(-1, keepdim=True)
        py = (p * onehot).sum(-1, keepdim=True)
        g = om.pow(gamma) * (A * p - a) - ce * gamma * om.pow(gamma - 1.0) * py * (onehot - p)
    return g * live[:, None]


def ref_with_grads(z, labels, mask=None, weight=None, smoothing=0.0, gamma=0.0, reduction="mean", B=1, scale=1.0):
    """-> (loss, rows, d(UPSTREAM * loss)/dz), all float64, by autograd"""
    zd = z.double().clone().requires_grad_(True)
    loss, rows = token_ce_ref(zd, labels, mask, weight, smoothing, gamma, reduction, B, scale)
    (gz,) = torch.autograd.grad(UPSTREAM * loss, (zd,), allow_unused=True)
    return loss.detach(), rows.detach(), torch.zeros_like(zd) if gz is None else gz


@functools.lru_cache(maxsize=None)
def reference(shape, mask_name, weighted, smoothing, gamma, reduction):
    """One case: computed once, shared, not to be modified.  -> (z, labels, mask, weight, loss, rows, gz)"""
    N, C = shape
    z, labels, mask = make_logits(N, C), make_labels(N, C), make_mask(mask_name, N)
    weight = make_weights(C) if weighted else None
    return (z, labels, mask, weight) + ref_with_grads(z, labels, mask, weight, smoothing, gamma, reduction, BATCH[N])


def extreme_logits(C=11, big=1e4):
    """Rows +-big * one-hot, the label on and off the marked tag -> (z [4,C], labels [4]).  Row 0: +big at the label (the peak);
    row 1: +big elsewhere; row 2: -big at the label (every other tag shares the mass); row 3: -big elsewhere."""
    z, y = torch.zeros(4, C), torch.tensor([2, 3, 4, 5])
    z[0, 2], z[1, 7], z[2, 4], z[3, 8] = big, big, -big, -big
    return z, y


def tied_logits(N, C, seed=3):
    """Logits on a coarse grid (many exact ties inside a row), plus rows that are constant."""
    g = torch.Generator().manual_seed(seed + 100 * N + C)
    z = torch.randint(-2, 3, (N, C), generator=g).float()
    z[::7] = 1.5
    return z
