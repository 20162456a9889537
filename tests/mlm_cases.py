"""NumPy restatements of the masked-LM kernels' contracts (csrc/mlm.hip), shared by tests/test_mlm.py (CPU) and
tests/test_mlm_gpu.py: the masking rule with its compaction, and the cross entropy over a chunked vocabulary in float64."""
from __future__ import annotations

import numpy as np


def mask_reference(ids, attention_mask, uniforms, probability, mask_token_id, V, special_ids=(), special_mask=None, capacity=None):
    """-> ids_out [B,S] int64, positions [capacity] int32, labels [capacity] int64, count, stats (eligible, selected, dropped).
    The fp32 comparisons and the fp32 product u2 * V are the kernel's."""
    ids = np.asarray(ids, dtype=np.int64)
    B, S = ids.shape
    u = np.asarray(uniforms, dtype=np.float32).reshape(B, S, 3)
    capacity = B * S if capacity is None else capacity
    elig = np.asarray(attention_mask).reshape(B, S) != 0
    if special_mask is not None:
        elig &= np.asarray(special_mask).reshape(B, S) == 0
    for s in special_ids:
        elig &= ids != s
    sel = elig & (u[..., 0] < np.float32(probability))
    out = ids.copy()
    positions = np.full(capacity, -1, dtype=np.int32)
    labels = np.full(capacity, -100, dtype=np.int64)
    n = 0
    for b in range(B):  # row-major order
        for t in range(S):
            if not sel[b, t]:
                continue
            if n < capacity:
                positions[n], labels[n] = b * S + t, ids[b, t]
                if u[b, t, 1] < np.float32(0.8):
                    out[b, t] = mask_token_id
                elif u[b, t, 1] < np.float32(0.9):
                    out[b, t] = min(V - 1, int(np.float32(u[b, t, 2]) * np.float32(V)))
            n += 1
    count = min(n, capacity)
    return out, positions, labels, count, np.array([int(elig.sum()), n, n - count], dtype=np.int32)


def _live(labels, count, V):
    labels = np.asarray(labels, dtype=np.int64)
    return (np.arange(labels.size) < count) & (labels >= 0) & (labels < V)


def ce_oneshot(logits, labels, count, reduction="mean"):
    """float64 cross entropy over whole rows.  -> dict(loss, loss_row, lse_row, argmax (first maximum), live, correct)."""
    z = np.asarray(logits, dtype=np.float64)
    R, V = z.shape
    live = _live(labels, count, V)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    arg = z.argmax(1)  # numpy: the first maximum
    lab = np.where(live, labels, 0)
    rows = np.where(live, lse - z[np.arange(R), lab], 0.0)
    n = int(live.sum())
    total = float(rows.sum())
    loss = (total / n if reduction == "mean" else total) if n else 0.0
    return {"loss": loss, "loss_row": rows, "lse_row": np.where(live, lse, 0.0), "argmax": arg, "live": n,
            "correct": int((live & (arg == labels)).sum())}


def ce_chunked(logits, labels, count, chunk, reduction="mean"):
    """The kernels' recurrence in float64: per chunk the maximum with its first index and s_c = sum exp(l - m_c); merged into
    (m, s, arg) with one rescale, chunks ascending, a later chunk replacing arg only if its maximum is GREATER."""
    z = np.asarray(logits, dtype=np.float64)
    R, V = z.shape
    live = _live(labels, count, V)
    m = np.full(R, -np.inf)
    s = np.zeros(R)
    arg = np.zeros(R, dtype=np.int64)
    for v0 in range(0, V, chunk):
        c = z[:, v0:v0 + chunk]
        mc, ac = c.max(1), c.argmax(1)
        sc = np.exp(c - mc[:, None]).sum(1)
        grow = mc > m
        with np.errstate(invalid="ignore", over="ignore"):  # (the branch np.where does not take, at m = -inf)
            s = np.where(grow, s * np.where(np.isinf(m), 0.0, np.exp(m - mc)) + sc, s + sc * np.exp(mc - m))
        arg = np.where(grow, v0 + ac, arg)
        m = np.where(grow, mc, m)
    lse = m + np.log(s)
    lab = np.where(live, labels, 0)
    rows = np.where(live, lse - z[np.arange(R), lab], 0.0)
    n = int(live.sum())
    total = float(rows.sum())
    loss = (total / n if reduction == "mean" else total) if n else 0.0
    return {"loss": loss, "loss_row": rows, "lse_row": np.where(live, lse, 0.0), "argmax": arg, "live": n,
            "correct": int((live & (arg == labels)).sum())}


def ce_grad_logits(logits, labels, count, g_rows):
    """d loss / d logits in float64 for per-row upstream gradients g_rows (mean: 1 / live on every row)."""
    z = np.asarray(logits, dtype=np.float64)
    R, V = z.shape
    live = _live(labels, count, V)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    lab = np.where(live, labels, 0)
    p[np.arange(R), lab] -= 1.0
    return p * (np.asarray(g_rows, dtype=np.float64) * live)[:, None]
