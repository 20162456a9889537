"""Time of the gradient-norm launches of the clipped AdamW step (csrc/gradnorm.hip) against the bytes they read, on the gradient set
of the headline configuration (BERT-base: twelve per-layer flat buffers of 7,087,872 floats, the embedding tables, pooler and
heads -- 109.5 M floats, 438 MB).  HIP events around `--iters` repetitions after `--warmup`; prints one JSON line.

    python tools/gradnorm_time.py [--iters 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYER = 3 * 768 * 768 + 3 * 768 + 768 * 768 + 768 + 2 * 768 + 2 * 768 * 3072 + 3072 + 768 + 2 * 768
OTHERS = [30522 * 768, 512 * 768, 2 * 768, 768, 768, 768 * 768, 768, 10 * 768, 10, 100, 10, 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from mtvaf_amd import hip
    assert LAYER == 7087872
    grads = [torch.randn(LAYER, device="cuda") * 1e-3 for _ in range(12)] + [torch.randn(n, device="cuda") * 1e-3 for n in OTHERS]
    nbytes = 4 * sum(t.numel() for t in grads)
    part = torch.empty(hip.grad_sqnorm_slots(grads), dtype=torch.float64, device="cuda")
    state = torch.zeros(4, device="cuda")
    skipped = torch.zeros((), dtype=torch.int32, device="cuda")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters  # us per repetition

    t_norm = timed(lambda: hip.grad_sqnorm(grads, part))
    t_fin = timed(lambda: hip.grad_clip_finalize(part, 1.0, state, skipped))
    t_both = timed(lambda: hip.grad_clip_finalize(hip.grad_sqnorm(grads, part), 1.0, state, skipped))
    ref = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    print(json.dumps({"tensors": len(grads), "bytes_read": nbytes, "partials": part.numel(), "sqnorm_us": round(t_norm, 2),
                      "sqnorm_TBps": round(nbytes / t_norm / 1e6, 3), "finalize_us": round(t_fin, 2),
                      "norm_and_finalize_us": round(t_both, 2), "norm": float(state[0]), "norm_float64_torch": ref,
                      "iters": a.iters}))


if __name__ == "__main__":
    main()
