"""Times `CalibrationScorer.update_events` (mtvaf_chunk_calibration: two launches, no host read) beside the eager path it replaces at
one shape: `.cpu()` of log_post, the labels, the mask and the kept columns, the Python chunker and a NumPy histogram.

    python tools/calibration_bench.py [--batch 32 --seq 128 --width 8 --bins 20 --iters 200 --host-iters 20 --repeats 7]

Labels O, B- / I- of two entity types and X: four types under the "seqeval" tables (PAD's, the one of O and X, and the two
entity types).  log_post is random, not a chain's: about a third of the events at kept start columns are finite, every type
alike.  One process: a warm-up of every path,
then ``--repeats`` timed windows of each, alternating; the median and the min-max of the windows are printed.  Device side: HIP
events around ``--iters`` back-to-back updates, and the wall time of one update followed by a synchronize.  Host side: the wall
time of the whole eager path on the same tensors.  Before anything is timed the two paths must agree on every integer counter."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_update(acc, log_post, keep, labels, mask, tables, edges, W):
    """The eager alternative: four device->host copies, a Python chunker over the two tables, NumPy masks and a histogram.
    acc = [n, hit, gold, reach, sum_p, sum_sq] arrays, added into."""
    import calibration_cases as K
    lp, kp, gold, msk = log_post.cpu().numpy(), keep.cpu().numpy(), labels.cpu().numpy(), mask.cpu().numpy()
    start, end, type_of = tables
    n_labels, (B, S, _, T), NB = len(type_of) - 1, lp.shape, len(edges) - 1
    y = np.zeros(lp.shape, dtype=bool)
    for s in range(B):
        cols = K.kept_columns(msk[s], kp[s])
        for t, b, e in K.gold_chunks(gold[s], cols, start, end, type_of, n_labels):
            acc[2][t] += 1
            if e - b < W:
                acc[3][t] += 1
                y[s, cols[b], e - b, t] = True
    finite = lp > -np.inf
    bins = (lp[..., None] >= edges[1:NB]).sum(-1)
    p = np.exp(lp.astype(np.float64), where=finite, out=np.zeros(lp.shape))
    cell = (np.arange(T) * NB + bins)[finite]
    size = T * NB
    acc[0] += np.bincount(cell, minlength=size).reshape(T, NB)
    acc[1] += np.bincount(cell, weights=y[finite].astype(np.float64), minlength=size).astype(np.int64).reshape(T, NB)
    acc[4] += np.bincount(cell, weights=p[finite], minlength=size).reshape(T, NB)
    acc[5] += np.bincount(cell, weights=(p[finite] - y[finite].astype(np.float64)) ** 2, minlength=size).reshape(T, NB)


def summary(xs):
    return f"median {statistics.median(xs):9.1f}  min {min(xs):9.1f}  max {max(xs):9.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_bench: no GPU -- there is nothing to time without one")
    import calibration_cases as K
    from mtvaf_amd.metrics import CalibrationScorer, entity_tables
    B, S, W, dev = a.batch, a.seq, a.width, "cuda"
    lmap = {n: i for i, n in enumerate(["O", "B-POS", "I-POS", "B-NEG", "I-NEG", "X"], 1)}
    rng = np.random.default_rng(0)
    gold, mask = K.valid_bio(rng, dict(lmap, **{"[CLS]": lmap["X"], "[SEP]": lmap["X"]}), B, S)  # X stands at both ends
    sc = CalibrationScorer(lmap, n_bins=a.bins, device=dev)
    T = len(sc.types)
    t = entity_tables(lmap)
    tables, edges = (t["start"], t["end"], t["type_of"]), sc.edges.numpy()
    keep = np.cumprod(mask, axis=1).astype(bool) & (gold != lmap["X"])
    keep[:, 0] = False
    lp = np.log(rng.uniform(1e-6, 1.0, (B, S, W, T))).astype(np.float32)
    lp[rng.random(lp.shape) < 0.66] = -np.inf
    lp[~keep] = -np.inf
    lpt, kt, gt, mt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (lp, keep.astype(np.uint8), gold, mask))

    acc = [np.zeros((T, a.bins), np.int64), np.zeros((T, a.bins), np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64),
           np.zeros((T, a.bins)), np.zeros((T, a.bins))]
    host_update(acc, lpt, kt, gt, mt, tables, edges, W)
    sc.update_events(lpt, kt, gt, mt)
    n, hit, g, reach, sum_p, sum_sq, _ = (x.numpy() for x in sc._fields(sc.block.cpu()))
    assert all(np.array_equal(x, y) for x, y in zip((n, hit, g, reach), acc[:4])), "device and host paths disagree"
    assert np.allclose(sum_p, acc[4], rtol=1e-9, atol=0) and np.allclose(sum_sq, acc[5], rtol=1e-9, atol=0)
    print(f"B {B} S {S} W {W} T {T} NB {a.bins}: {int(n.sum())} finite events of {lp.size}, {int(hit.sum())} hits, "
          f"{int(g.sum())} gold chunks per batch")

    def device_window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            sc.update_events(lpt, kt, gt, mt)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def sync_window():
        t0 = time.perf_counter()
        for _ in range(a.iters):
            sc.update_events(lpt, kt, gt, mt)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.iters

    def host_window():
        t0 = time.perf_counter()
        for _ in range(a.host_iters):
            host_update(acc, lpt, kt, gt, mt, tables, edges, W)
        return (time.perf_counter() - t0) * 1e6 / a.host_iters

    for f in (device_window, sync_window, host_window):  # warm-up of every path
        f()
    dev_us, sync_us, host_us = [], [], []
    for _ in range(a.repeats):  # alternating windows
        dev_us.append(device_window())
        sync_us.append(sync_window())
        host_us.append(host_window())
    print(f"update_events               {summary(dev_us)}  us per call (device events, back-to-back calls, {a.repeats} windows)")
    print(f"update_events + sync        {summary(sync_us)}  us per call (wall)")
    print(f"host copy + chunk + bincount{summary(host_us)}  us per batch (wall, {a.host_iters} runs per window)")


if __name__ == "__main__":
    main()
