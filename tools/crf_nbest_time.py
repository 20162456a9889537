"""Times `mtvaf_crf_nbest` for K = 1, 4, 8 beside `mtvaf_crf_viterbi` on the same batch: what K costs relative to one-best.

    python tools/crf_nbest_time.py [--batch 32 --seq 128 --tags 13 --iters 200]

HIP events around back-to-back calls into preallocated outputs (`hip.crf_nbest(..., out=...)`; the workspace comes from torch's
caching allocator), full-length sentences.  Each K is timed with the log-probabilities (forward recursion + n-best kernel) and
without them (the n-best kernel alone).  No threshold: the figures go into DESIGN.md section 4.11."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--tags", type=int, default=13)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from mtvaf_amd import hip
    B, S, C, dev = a.batch, a.seq, a.tags, "cuda"
    g = torch.Generator().manual_seed(0)
    em = (torch.randn(B, S, C, generator=g) * 2).to(dev)
    start, end, trans = ((torch.rand(*s, generator=g) - 0.5).to(dev) for s in ((C,), (C,), (C, C)))
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    tags1 = torch.empty(B, S, dtype=torch.int32, device=dev)
    lens1 = torch.empty(B, dtype=torch.int32, device=dev)
    base = timed(lambda: hip.crf_viterbi(em, mask, start, end, trans, tags1, lens1), a.iters)
    print(f"B {B} S {S} C {C}, us per call (device events, {a.iters} back-to-back calls)")
    print(f"mtvaf_crf_viterbi            {base:9.1f}")
    for K in (1, 4, 8):
        out = (torch.empty(B, K, S, dtype=torch.int32, device=dev), torch.empty(B, K, device=dev), torch.empty(B, K, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
        full = timed(lambda: hip.crf_nbest(em, mask, start, end, trans, K, out=out), a.iters)
        bare = timed(lambda: hip.crf_nbest(em, mask, start, end, trans, K, out=(out[0], out[1], None, out[3])), a.iters)
        assert torch.equal(out[0][:, 0], tags1), "rank 0 is not the one-best path"
        print(f"mtvaf_crf_nbest K = {K}        {full:9.1f}  ({full / base:5.1f} x one-best)   without logprob {bare:9.1f}  "
              f"({bare / base:5.1f} x)")


if __name__ == "__main__":
    main()
