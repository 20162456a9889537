"""Times `EntityScorer.update` (mtvaf_entity_counts, one launch) beside the per-step host path it replaces at one shape.

    python tools/entity_score_time.py [--batch 32 --seq 128 --iters 200 --host-iters 20]

Device side: HIP events around back-to-back `update` calls, and the wall time of one call followed by a synchronize.  Host side,
on the same batch: `mtvaf_amd.metrics.label_sequences` (two blocking `.to("cpu")` copies, the packed tag copy through
`CRF`'s `DeferredTags`, object-array indexing) as wall time; the string chunking at epoch end is not in the host figure."""
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=20)
    a = ap.parse_args()
    import entity_cases as E
    from mtvaf_amd.metrics import EntityScorer, label_sequences
    from mtvaf_amd.modules.crf import DeferredTags
    B, S, dev = a.batch, a.seq, "cuda"
    lmap = E.label_map("a")
    gold, pred, mask = E.make_case(np.random.default_rng(0), lmap, B, S, "ragged", "mixed", 0.3)
    gt, pt, mt = (torch.from_numpy(x).to(dev) for x in (gold, pred, mask))
    lens = torch.from_numpy(mask.sum(1).astype(np.int32)).to(dev)
    sc = EntityScorer(lmap, device=dev)

    def host_path():  # what a step pays today: the packed copy decode_deferred enqueues, then label_sequences
        packed = torch.cat([pt, lens[:, None]], 1).to("cpu", non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return label_sequences(gt, mt, DeferredTags(packed, ev, S), lmap)

    sc.update(pt, gt, mt)
    y_true, y_pred = host_path()
    as_labels = lambda rows: [[(n, n == "O") for n in row] for row in rows]  # noqa: E731
    want = E.counter(sc.types, E.count_sequences("seqeval", as_labels(y_true), as_labels(y_pred)))
    assert sc.counts.cpu().numpy().tolist() == want.tolist(), "device and host paths disagree"
    for _ in range(10):
        sc.update(pt, gt, mt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        sc.update(pt, gt, mt)
    e1.record()
    torch.cuda.synchronize()
    dev_us = e0.elapsed_time(e1) * 1e3 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.iters):
        sc.update(pt, gt, mt)
        torch.cuda.synchronize()
    sync_us = (time.perf_counter() - t0) * 1e6 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.host_iters):
        host_path()
    host_us = (time.perf_counter() - t0) * 1e6 / a.host_iters
    print(f"B {B} S {S}: {int(want[-1])} kept tokens, {int(want[1:-2:3].sum())} gold entities per batch")
    print(f"EntityScorer.update         {dev_us:10.1f} us per call (device events, back-to-back calls)")
    print(f"EntityScorer.update + sync  {sync_us:10.1f} us per call (wall)")
    print(f"label_sequences             {host_us:10.1f} us per batch (wall, {a.host_iters} runs)")


if __name__ == "__main__":
    main()
