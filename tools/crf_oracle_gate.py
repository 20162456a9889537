"""The CRF a user would otherwise write: the oracle's crf_log_likelihood + backward + crf_decode as torch ops on GPU tensors
in fp32, against the HIP kernels (mtvaf_crf_nll_fwd + _bwd + _viterbi) on the same inputs.
    python tools/crf_oracle_gate.py B C [S ...]      (default S: 128 512)
Prints one line per S: milliseconds per call of both and their ratio."""
import sys
import time

import torch

sys.path[:0] = ["."]
from mtvaf_amd import hip  # noqa: E402
from oracle import mtvaf_oracle as O  # noqa: E402

B, C = int(sys.argv[1]), int(sys.argv[2])
Ss = [int(s) for s in sys.argv[3:]] or [128, 512]
dev = "cuda:0"
g = torch.Generator().manual_seed(0)
for S in Ss:
    em = torch.randn(B, S, C, generator=g).to(dev)
    tags = torch.randint(0, C, (B, S), generator=g).to(dev)
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    start, end, trans = (torch.rand(n, generator=g).sub(0.5).to(dev) for n in ((C,), (C,), (C, C)))

    def torch_ops():
        e, s, en, t = (x.clone().requires_grad_(True) for x in (em, start, end, trans))
        (-O.crf_log_likelihood(e, tags, mask, s, en, t, "mean")).backward()
        O.crf_decode(em, mask, start, end, trans)
        torch.cuda.synchronize()

    ws, wsb = hip.crf_workspace(B, S, C, dev)
    loss = torch.empty(1, device=dev)
    dem = torch.empty(B, S, C, device=dev)
    ds, de, dt = (torch.zeros(n, device=dev) for n in ((C,), (C,), (C, C)))
    tg, ln = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)

    def kernels():
        hip.crf_nll_fwd(em, tags, mask, start, end, trans, loss, ws, wsb)
        hip.crf_nll_bwd(None, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws, wsb)
        hip.crf_viterbi(em, mask, start, end, trans, tg, ln)
        torch.cuda.synchronize()

    res = {}
    for name, fn, n in (("torch_ops", torch_ops, 2), ("kernels", kernels, 20)):
        fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        res[name] = (time.perf_counter() - t0) * 1e3 / n
    print(f"B={B} S={S} C={C}: torch ops {res['torch_ops']:.2f} ms, kernels {res['kernels']:.3f} ms, "
          f"ratio {res['torch_ops'] / res['kernels']:.0f}x", flush=True)
