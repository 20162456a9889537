"""Measurements of the word-level head's kernels on one MI355X:

    python tools/wordpool_bench.py [--rounds 20] [--reps 100] [--out profiles/wordpool_bench.json]

Index + forward + backward (mtvaf_word_index, mtvaf_word_pool_fwd, mtvaf_word_pool_bwd) at the headline shape (32 x 128 x 768,
bench.py's ragged lengths, words of 1 - 4 pieces, half of them one piece; the pieces per column are reported) against the eager chain they replace -- the
column of every token by `cumsum`, `index_add_` of the piece rows (float atomics), the division by the counts, the gather
backward through autograd -- which also needs the widest sentence on the host to size the axis; here it is given the width for
free.  The two take turns; device events around `reps` back-to-back calls; reported: median, min and max over the rounds."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
DEV = "cuda:0"


def word_map(mask, seed=0):
    """[CLS], words of 1 - 4 pieces (half of them one piece), [SEP] per sentence; -1 outside the map."""
    gen = torch.Generator().manual_seed(seed)
    B, S = mask.shape
    t2w = torch.full((B, S), -1, dtype=torch.int32)
    for b, n in enumerate(mask.sum(1).tolist()):
        s, w = 1, 0
        while s < n - 1:
            k = int(torch.tensor([1, 1, 1, 1, 2, 2, 3, 4])[torch.randint(0, 8, (1,), generator=gen)])
            t2w[b, s:min(s + k, n - 1)] = w
            s, w = s + k, w + 1
    return t2w


def eager_index(mask, t2w):
    live = torch.cumprod(mask.ne(0).long(), dim=1).bool()
    m = torch.where(live, t2w.long(), torch.full((), -1, dtype=torch.long, device=mask.device))
    prev = torch.cat([torch.full_like(m[:, :1], -1), m[:, :-1]], dim=1)
    opens = live & ((m < 0) | (m != prev))
    opens[:, 0] = live[:, 0]
    col = torch.cumsum(opens.long(), dim=1) - 1
    return torch.where(live, col, torch.full_like(col, -1)), live


def eager_mean(x, col, live, W):
    B, S, H = x.shape
    flat = (col + torch.arange(B, device=x.device)[:, None] * W)[live]
    y = torch.zeros(B * W, H, device=x.device).index_add_(0, flat, x[live])
    n = torch.zeros(B * W, device=x.device).index_add_(0, flat, torch.ones(flat.numel(), device=x.device))
    return (y / n.clamp_min(1)[:, None]).view(B, W, H)


def run(rounds, reps, warmup=20):
    import bench
    from mtvaf_amd import hip
    from mtvaf_amd.words import WordPooling, build_word_index
    B, S, H = 32, 128, 768
    mask = bench.synthetic_batch(B, S, 8, 30522, 1234, DEV)[1]
    t2w = word_map(mask.cpu()).to(DEV)
    m8 = hip.adv_mask(mask)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, S, H, generator=gen).to(DEV).requires_grad_(True)
    dy = torch.randn(B, S, H, generator=gen).to(DEV)
    pool = WordPooling("mean")

    def kernels():
        index = build_word_index(m8, t2w)
        pool(x, index).backward(dy)
        x.grad = None

    def eager():
        col, live = eager_index(mask, t2w)
        eager_mean(x, col, live, S).backward(dy)
        x.grad = None

    # the two agree (the eager sum's order is not fixed: compare to rounding, not bits)
    index = build_word_index(m8, t2w)
    col, live = eager_index(mask, t2w)
    a, b = pool(x, index).detach(), eager_mean(x, col, live, S).detach()
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    fns = {"index_fwd_bwd_kernels": kernels, "index_fwd_bwd_eager_torch": eager}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    res = {n: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "rounds": len(v),
               "calls_per_round": reps} for n, v in times.items()}
    tokens, words = int(index.col_of_token.ge(0).sum()), int(index.word_mask.sum())
    # forward: the live piece rows in, every column row out; backward: the live columns' dy in, every token row out
    res.update(live_tokens=tokens, words=words, pieces_per_word=round(tokens / words, 3),
               bytes_fwd_bwd=(tokens + B * S) * H * 4 + (words + B * S) * H * 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0), **run(a.rounds, a.reps)}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
