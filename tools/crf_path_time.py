"""Times `mtvaf_crf_path_fwd + mtvaf_crf_path_bwd` (node and edge cost, no dcost / decost: the entropy's pair of calls) beside
`mtvaf_crf_risk_fwd + mtvaf_crf_risk_bwd` on the same batch: what the edge term costs on top of a column-additive cost.

    python tools/crf_path_time.py [--batch 32 --seq 128 --tags 13 64 --window 0.5 --repeats 7]

The method is tools/crf_risk_time.py's: HIP events around back-to-back calls into preallocated outputs and workspaces, full-length
sentences; after a warm-up the number of pairs per window is set so that a window lasts about ``--window`` seconds; the two
variants are timed ALTERNATELY, window by window, and the median of the windows is reported with their spread.  What bounds
either pair is not measured here: no trace is taken.  No threshold: the figures go into DESIGN.md section 4.15."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.crf_risk_time import timed_alternately  # noqa: E402


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
        ecost = torch.randn(C, C, generator=g).to(dev)
        start, end, trans = ((torch.rand(*s, generator=g) - 0.5).to(dev) for s in ((C,), (C,), (C, C)))
        mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
        w = torch.ones(B, device=dev)
        out, dem = torch.empty(B, device=dev), torch.empty(B, S, C, device=dev)
        ds, de, dt = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(C, C, device=dev)
        ws_r, wsb_r = hip.crf_risk_workspace(B, S, C, dev)
        ws_p, wsb_p = hip.crf_path_workspace(B, S, C, dev)

        def risk():
            hip.crf_risk_fwd(em, cost, mask, start, end, trans, out, None, None, ws_r, wsb_r)
            hip.crf_risk_bwd(w, em, cost, mask, start, end, trans, dem, None, ds, de, dt, False, ws_r, wsb_r)

        def path():
            hip.crf_path_fwd(em, cost, ecost, mask, start, end, trans, out, None, ws_p, wsb_p)
            hip.crf_path_bwd(w, None, em, cost, ecost, mask, start, end, trans, dem, None, None, ds, de, dt, False, ws_p, wsb_p)

        (r, p), iters = timed_alternately((risk, path), a.window, a.repeats)
        print(f"C {C:3d}  mtvaf_crf_risk_fwd + bwd  {r[0]:8.1f} [{r[1]:.1f}, {r[2]:.1f}]   mtvaf_crf_path_fwd + bwd  {p[0]:8.1f} "
              f"[{p[1]:.1f}, {p[2]:.1f}]   ratio {p[0] / r[0]:.2f}   (pairs per window {iters[0]}, {iters[1]})")


if __name__ == "__main__":
    main()
