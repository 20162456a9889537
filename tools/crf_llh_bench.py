"""Cost of the per-sentence CRF entry points and the marginals against the NLL pair of the same build, by HIP events:
variants interleaved in rounds inside one process, median and minimum per variant (us per call, back-to-back launches).
    python tools/crf_llh_bench.py [B] [S] [rounds]        (C = 11 and C = 64)"""
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
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    start, end, trans = (torch.rand(n, generator=g).sub(0.5).to(dev) for n in ((C,), (C,), (C, C)))
    ws, wsb = hip.crf_workspace(B, S, C, dev)
    loss, llh, w = torch.empty(1, device=dev), torch.empty(B, device=dev), torch.randn(B, generator=g).to(dev)
    dem, marg = torch.empty(B, S, C, device=dev), torch.empty(B, S, C, device=dev)
    ds, de, dt = (torch.zeros(n, device=dev) for n in ((C,), (C,), (C, C)))
    nll_fwd = lambda: hip.crf_nll_fwd(em, tags, mask, start, end, trans, loss, ws, wsb)
    nll_bwd = lambda: hip.crf_nll_bwd(None, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws, wsb)
    llh_fwd = lambda: hip.crf_llh_fwd(em, tags, mask, start, end, trans, llh, ws, wsb)
    llh_bwd = lambda: hip.crf_llh_bwd(w, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws, wsb)
    fns = {"nll_fwd+nll_bwd": lambda: (nll_fwd(), nll_bwd()), "llh_fwd+llh_bwd": lambda: (llh_fwd(), llh_bwd()),
           "nll_bwd": nll_bwd, "marginals": lambda: hip.crf_marginals(em, mask, start, end, trans, marg, llh, ws, wsb)}
    times = {k: [] for k in fns}
    nll_fwd()  # (the backward-only variant reads this forward's workspace)
    for r in range(ROUNDS + 1):
        for name, fn in fns.items():
            if name == "nll_bwd":
                nll_fwd()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:  # round 0 warms up
                times[name].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    for name, t in times.items():
        print(f"B={B} S={S} C={C} {name:16s} median {statistics.median(t):7.2f} us  min {min(t):7.2f} us", flush=True)
