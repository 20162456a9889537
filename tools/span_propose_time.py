"""Times the candidate-span proposal (mtvaf_span_propose, one launch) beside the host path it replaces at one shape.

    python tools/span_propose_time.py [--batch 32 --seq 128 --n-best 20 --iters 200 --host-iters 5] [--nms]

Device side: HIP events around back-to-back `hip.span_propose` calls (output allocation included), and the wall time of one
call followed by a synchronize.  Host side, on the same logits: what the reference's trainer does between `extraction` and
`classification` (modules/train.py:382-410) -- two `.cpu().tolist()` per sentence, the rule as a Python loop
(tests/span_propose_cases.py, the restatement the tests use; the reference additionally builds and normalises a text per
candidate), four `torch.tensor(...)` and four copies to the device -- as wall time up to a final synchronize."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--n-best", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=12)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--nms", action="store_true")
    a = ap.parse_args()
    from mtvaf_amd import hip
    import span_propose_cases as C
    B, S, n_best, dev = a.batch, a.seq, a.n_best, "cuda"
    sl, el, wi, wk = C.make_inputs(B, S, seed=0)
    ae = torch.from_numpy(np.stack([sl, el], -1)).to(dev)
    wit, wkt = torch.from_numpy(wi).to(dev), torch.from_numpy(wk).to(dev)
    kw = dict(n_best=n_best, max_len=a.max_len, threshold=C.THRESHOLD, use_heuristics=True, nms=int(a.nms))

    def device_path():
        return hip.span_propose(ae, wit, wkt, **kw)

    def host_path():
        rows = []
        for b in range(B):
            s_row, e_row = ae[b, :, 0].detach().cpu().tolist(), ae[b, :, 1].detach().cpu().tolist()
            rows.append(C.propose_row(s_row, e_row, wi[b], wk[b], n_best, a.max_len, C.THRESHOLD, True, int(a.nms)))
        outs = [torch.tensor([r[k] for r in rows], dtype=torch.long).to(dev) for k in range(3)]
        outs.append(torch.tensor([[0] * n_best for _ in rows], dtype=torch.long).to(dev))  # the labels list
        torch.cuda.synchronize()
        return outs

    got, ref = device_path(), host_path()
    assert all(torch.equal(g, r) for g, r in zip(got[:3], ref[:3])), "device and host paths disagree"
    for _ in range(10):
        device_path()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        device_path()
    e1.record()
    torch.cuda.synchronize()
    dev_us = e0.elapsed_time(e1) * 1e3 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.iters):
        device_path()
        torch.cuda.synchronize()
    sync_us = (time.perf_counter() - t0) * 1e6 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.host_iters):
        host_path()
    host_us = (time.perf_counter() - t0) * 1e6 / a.host_iters
    print(f"B {B} S {S} n_best {n_best} max_len {a.max_len} nms {int(a.nms)}: accepted {int(got[4].sum())} spans")
    print(f"span_propose            {dev_us:10.1f} us per call (device events, back-to-back calls)")
    print(f"span_propose + sync     {sync_us:10.1f} us per call (wall)")
    print(f"host path it replaces   {host_us:10.1f} us per batch (wall, {a.host_iters} runs)")


if __name__ == "__main__":
    main()
