"""Times `SpanScorer.update` (mtvaf_span_counts, one launch) beside the per-batch host path it replaces at one shape.

    python tools/span_score_time.py [--batch 32 --seq 128 --n-best 20 --gold 4 --iters 200 --host-iters 20]

Device side: HIP events around back-to-back `update` calls, and the wall time of one call followed by a synchronize.  Host side,
on the same tensors: the per-sentence copies of the reference trainer's eval loop (modules/train.py:200-209: the class logits'
arg-max and the span lists of every sentence through `.cpu().tolist()`), the gold lists and word maps the same way, then the
counting loop of the restatement (tests/span_score_cases.py) as wall time; the reference additionally builds and normalises a
text per span, which is not in the host figure."""
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
    ap.add_argument("--gold", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=20)
    a = ap.parse_args()
    import span_score_cases as C
    from mtvaf_amd.metrics import SpanScorer
    B, S, N, G, K, dev = a.batch, a.seq, a.n_best, a.gold, 4, "cuda"
    inp = C.make_inputs(B, S, N, G, K, seed=0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    pred = {k: t[k] for k in ("span_starts", "span_ends", "label_masks", "logits")}
    gold = [t[k] for k in ("gold_starts", "gold_ends", "gold_class", "gold_masks")]
    sc = SpanScorer(device=dev)

    def update():
        sc.update(pred, *gold, t["word_index"], t["word_key"])

    def host_path():  # what a batch pays today: per-sentence copies, then the counting loop
        rows = {k: [] for k in inp}
        for j in range(B):
            rows["logits"].append(t["logits"][j].detach().cpu().numpy())
            for k in inp:
                if k != "logits":
                    rows[k].append(t[k][j].detach().cpu().tolist())
        return C.score(**{k: np.array(v) for k, v in rows.items()})

    update()
    want = host_path()["counts"]
    assert sc.counts.cpu().numpy().tolist() == want.tolist(), "device and host paths disagree"
    for _ in range(10):
        update()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        update()
    e1.record()
    torch.cuda.synchronize()
    dev_us = e0.elapsed_time(e1) * 1e3 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.iters):
        update()
        torch.cuda.synchronize()
    sync_us = (time.perf_counter() - t0) * 1e6 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.host_iters):
        host_path()
    host_us = (time.perf_counter() - t0) * 1e6 / a.host_iters
    common, retrieved, relevant = C.totals(want, K)
    print(f"B {B} S {S} n_best {N} G {G}: {retrieved} predicted, {relevant} gold, {common} common terms per batch")
    print(f"SpanScorer.update           {dev_us:10.1f} us per call (device events, back-to-back calls)")
    print(f"SpanScorer.update + sync    {sync_us:10.1f} us per call (wall)")
    print(f"host copies + counting loop {host_us:10.1f} us per batch (wall, {a.host_iters} runs)")


if __name__ == "__main__":
    main()
