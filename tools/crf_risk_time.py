"""Times `mtvaf_crf_risk_fwd + mtvaf_crf_risk_bwd` beside `mtvaf_crf_llh_fwd + mtvaf_crf_llh_bwd` on the same batch: what the
gradient of a posterior expectation costs relative to the gradient of the likelihood.

    python tools/crf_risk_time.py [--batch 32 --seq 128 --tags 13 64 --window 0.5 --repeats 7]

HIP events around back-to-back calls into preallocated outputs and workspaces, full-length sentences.  After a warm-up the number
of pairs per window is set so that a window lasts about ``--window`` seconds (a window of a few milliseconds measures the clock
and the scheduler); the two variants are timed ALTERNATELY, window by window, so that a drift of the box falls on both, and the
median of the windows is reported with their spread.  What bounds either pair at these sizes (launch overhead of its launches,
or the latency of the serial chain of S steps in 32 one-wave blocks) is not measured here: no trace is taken.  No threshold: the
figures go into DESIGN.md section 4.14."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed_alternately(fns, seconds, repeats):
    """us per call of each function: median, min and max over ``repeats`` windows of about ``seconds`` each, taken in turn."""
    iters = []
    for fn in fns:
        window(fn, 50)
        iters.append(max(50, int(seconds * 1e6 / window(fn, 200))))
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, iters[k]))
    return [(statistics.median(o), min(o), max(o)) for o in out], iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--tags", type=int, nargs="+", default=[13, 64])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from mtvaf_amd import hip
    B, S, dev = a.batch, a.seq, "cuda"
    print(f"B {B} S {S}, us per fwd + bwd pair (device events, median [min, max] of {a.repeats} windows of about {a.window} s each, "
          f"the two variants in turn)")
    for C in a.tags:
        g = torch.Generator().manual_seed(0)
        em = (torch.randn(B, S, C, generator=g) * 2).to(dev)
        cost = torch.randn(B, S, C, generator=g).to(dev)
        tags = torch.randint(0, C, (B, S), generator=g).to(dev)
        start, end, trans = ((torch.rand(*s, generator=g) - 0.5).to(dev) for s in ((C,), (C,), (C, C)))
        mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
        w = torch.ones(B, device=dev)
        out, dem = torch.empty(B, device=dev), torch.empty(B, S, C, device=dev)
        ds, de, dt = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(C, C, device=dev)
        ws_l, wsb_l = hip.crf_workspace(B, S, C, dev)
        ws_r, wsb_r = hip.crf_risk_workspace(B, S, C, dev)

        def llh():
            hip.crf_llh_fwd(em, tags, mask, start, end, trans, out, ws_l, wsb_l)
            hip.crf_llh_bwd(w, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws_l, wsb_l)

        def risk():
            hip.crf_risk_fwd(em, cost, mask, start, end, trans, out, None, None, ws_r, wsb_r)
            hip.crf_risk_bwd(w, em, cost, mask, start, end, trans, dem, None, ds, de, dt, False, ws_r, wsb_r)

        (l, r), iters = timed_alternately((llh, risk), a.window, a.repeats)
        print(f"C {C:3d}  mtvaf_crf_llh_fwd + bwd  {l[0]:8.1f} [{l[1]:.1f}, {l[2]:.1f}]   mtvaf_crf_risk_fwd + bwd  {r[0]:8.1f} "
              f"[{r[1]:.1f}, {r[2]:.1f}]   ratio {r[0] / l[0]:.2f}   (pairs per window {iters[0]}, {iters[1]})")


if __name__ == "__main__":
    main()
