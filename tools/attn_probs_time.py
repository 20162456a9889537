"""Times the probabilities-on-request kernel (mtvaf_prefix_attn_probs) beside the forward attention kernel at one shape.

    python tools/attn_probs_time.py [--batch 32 --seq 128 --prefix 36 --heads 12 --iters 50] [--f32-pipe] [--full-length]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/attn_probs_time.py      # per-kernel times

Prints device-event times per launch and the probs kernel's bytes written / time (its floor is the HBM write of
B * NH * S * (P + S) * 4 bytes: 32 MB at the default, BASELINE config-2, shape)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--prefix", type=int, default=36)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--f32-pipe", action="store_true", help="the fp32 MFMA pipe instead of the split arithmetic")
    ap.add_argument("--full-length", action="store_true", help="no padding (default: lengths uniform in [S/4, S])")
    a = ap.parse_args()
    from mtvaf_amd import hip
    hip.f32_split(not a.f32_pipe)
    B, S, Pn, NH = a.batch, a.seq, a.prefix, a.heads
    H, dev = NH * 64, "cuda"
    rng = np.random.default_rng(0)
    qkv = torch.from_numpy(rng.standard_normal((B * S, 3 * H), dtype=np.float32)).to(dev)
    pk = torch.from_numpy(rng.standard_normal((B, max(Pn, 1) * H), dtype=np.float32)).to(dev)
    pv = pk.clone()
    lengths = [S] * B if a.full_length else [S] + [int(x) for x in rng.integers(max(2, S // 4), S + 1, size=B - 1)]
    mask = torch.zeros(B, Pn + S)
    mask[:, :Pn] = 1
    for b, n in enumerate(lengths):
        mask[b, Pn:Pn + n] = 1
    addmask = ((1.0 - mask) * -10000.0).to(dev)
    ctx, lse = torch.empty(B * S, H, device=dev), torch.empty(B, NH, S, device=dev)
    probs, mass = torch.empty(B, NH, S, Pn + S, device=dev), torch.empty(B, NH, S, device=dev)
    runs = {"forward (ctx, lse)": lambda: hip.prefix_attn_fwd(qkv, pk, pv, addmask, ctx, lse, B, S, Pn, NH, 0.0, 0, 0),
            "probs + prefix mass": lambda: hip.prefix_attn_probs(qkv, pk, addmask, probs, mass, B, S, Pn, NH),
            "prefix mass alone": lambda: hip.prefix_attn_probs(qkv, pk, addmask, None, mass, B, S, Pn, NH)}
    nbytes = probs.numel() * 4
    print(f"B {B} S {S} P {Pn} NH {NH}, {'fp32 pipe' if a.f32_pipe else 'split'} arithmetic, {sum(lengths)} of {B * S} tokens unmasked, "
          f"maps {nbytes / 1e6:.1f} MB")
    for name, fn in runs.items():
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        extra = f", {nbytes / us / 1e6:.2f} TB/s written" if name.startswith("probs") else ""
        print(f"{name:22s} {us:8.1f} us per launch (device events, back-to-back launches){extra}")


if __name__ == "__main__":
    main()
