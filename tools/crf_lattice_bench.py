"""Cost of the constrained CRF entry points against the unconstrained ones of the same build, by HIP events: variants
interleaved in rounds inside one process, 50 back-to-back calls per sample, median and minimum per variant (us per call) and the
ratio of each pair.  The sets are random with density 1/2 (the cost of a step does not depend on them).
    python tools/crf_lattice_bench.py [B] [S] [rounds]        (C = 11 and C = 64)
What to compare against: one constrained chain does the free chain's work per step (viterbi, marginals); the likelihood pair
runs two chains, the constrained and the free one, interleaved in one wave."""
import statistics
import sys

import torch

sys.path[:0] = ["."]
from mtvaf_amd import hip

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
S = int(sys.argv[2]) if len(sys.argv) > 2 else 128
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 21
CALLS = 50
dev = "cuda:0"
g = torch.Generator().manual_seed(0)
for C in (11, 64):
    em = torch.randn(B, S, C, generator=g).to(dev)
    tags = torch.randint(0, C, (B, S), generator=g).to(dev)
    allowed = (torch.randint(0, 1 << 31, (B, S), generator=g) | (torch.randint(0, 1 << 31, (B, S), generator=g) << 31)).to(dev)
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    start, end, trans = (torch.rand(n, generator=g).sub(0.5).to(dev) for n in ((C,), (C,), (C, C)))
    ws, wsb = hip.crf_workspace(B, S, C, dev)
    lws, lwsb = hip.crf_lattice_workspace(B, S, C, dev)
    llh, la, lz = (torch.empty(B, device=dev) for _ in range(3))
    w = torch.randn(B, generator=g).to(dev)
    dem, marg = torch.empty(B, S, C, device=dev), torch.empty(B, S, C, device=dev)
    ds, de, dt = (torch.zeros(n, device=dev) for n in ((C,), (C,), (C, C)))
    vt, vl = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    pairs = {
        "fwd+bwd": (lambda: (hip.crf_lattice_fwd(em, allowed, mask, start, end, trans, llh, la, lz, lws, lwsb),
                             hip.crf_lattice_bwd(w, em, allowed, mask, start, end, trans, dem, ds, de, dt, False, lws, lwsb)),
                    lambda: (hip.crf_llh_fwd(em, tags, mask, start, end, trans, llh, ws, wsb),
                             hip.crf_llh_bwd(w, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws, wsb))),
        "viterbi": (lambda: hip.crf_lattice_viterbi(em, allowed, mask, start, end, trans, vt, vl, llh),
                    lambda: hip.crf_viterbi(em, mask, start, end, trans, vt, vl)),
        "marginals": (lambda: hip.crf_lattice_marginals(em, allowed, mask, start, end, trans, marg, la, lws, lwsb),
                      lambda: hip.crf_marginals(em, mask, start, end, trans, marg, lz, ws, wsb)),
    }
    fns = {f"{side} {name}": fn for name, (lat, free) in pairs.items() for side, fn in (("lattice", lat), ("free", free))}
    times = {k: [] for k in fns}
    for r in range(ROUNDS + 1):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:  # round 0 warms up
                times[name].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    for name in pairs:
        lat, free = times[f"lattice {name}"], times[f"free {name}"]
        print(f"B={B} S={S} C={C} {name:10s} lattice median {statistics.median(lat):8.2f} us min {min(lat):8.2f} us | "
              f"free median {statistics.median(free):8.2f} us min {min(free):8.2f} us | ratio of medians "
              f"{statistics.median(lat) / statistics.median(free):5.2f}", flush=True)
