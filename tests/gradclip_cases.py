"""Shared by test_gradclip.py (host) and test_gradclip_gpu.py: a float64 restatement of "clip by global L2 norm, then AdamW" and
the case lists of the gradient-norm kernel.  No GPU, no library call.

The restatement: the norm is sqrt(sum of float64 squares) over every gradient that is applied; the coefficient is
torch.nn.utils.clip_grad_norm_'s, min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0); the update is the recurrence of the header
comment of csrc/optim.hip on g * coefficient."""
import math

import numpy as np
import torch

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
CHUNK = 65536  # elements per block of the sum-of-squares kernel (csrc/gradnorm.hip: SQ_CHUNK); one partial sum per chunk

# lengths of the tensors of the norm test: around the 256-lane block and its float4 body, one chunk exactly, one chunk + 1,
# 3 chunks + 5; ("view", n) is the [1:] view of a buffer of n + 1 floats -- 4-byte aligned, not 16 -- here longer than a chunk, so
# the scalar body also crosses a chunk edge
NORM_LENGTHS = [1, 3, 255, 256, 257, 1023, CHUNK, CHUNK + 1, 3 * CHUNK + 5, ("view", CHUNK + 77)]
# ... and enough small odd ones after them that one call carries more than the 48 tensors a launch takes
NORM_SMALL = [5 + 37 * i for i in range(45)]
assert len(NORM_LENGTHS) + len(NORM_SMALL) > 48 + 2


def norm_tensors(seed=7):
    """-> list of CPU fp32 tensors (randn) of the norm test, views included, in call order."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in NORM_LENGTHS + NORM_SMALL:
        if isinstance(n, tuple):
            out.append(torch.randn(n[1] + 1, generator=g)[1:])
        else:
            out.append(torch.randn(n, generator=g))
    return out


def expected_slots(lengths):
    return sum((n + CHUNK - 1) // CHUNK for n in lengths)


def global_norm(grads) -> float:
    """sqrt(sum float64(g)^2) over all tensors (numpy's pairwise float64 sum: error ~ log2(n) * 2^-53)."""
    return math.sqrt(sum(float(np.sum(np.square(t.detach().cpu().double().numpy()))) for t in grads))


def clip_coef(norm: float, max_norm: float) -> float:
    if max_norm <= 0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if c < 1.0 else 1.0


class ClipAdamW64:
    """groups: [{"params": [float64 tensors], "lr": .., "weight_decay": ..}, ...]; step(grads by id(param) or None entries)."""

    def __init__(self, groups, max_norm=0.0):
        self.groups = groups
        self.max_norm = max_norm
        self.state = {}
        self.norms = []

    def step(self, grads):
        """grads: list parallel to the flattened parameter list (None: the parameter is left out, also of the norm)."""
        flat = [p for g in self.groups for p in g["params"]]
        assert len(flat) == len(grads)
        norm = global_norm([g for g in grads if g is not None])
        coef = clip_coef(norm, self.max_norm)
        self.norms.append(norm)
        it = iter(grads)
        for group in self.groups:
            lr, wd = group["lr"], group["weight_decay"]
            for p in group["params"]:
                g = next(it)
                if g is None:
                    continue
                g = g.detach().cpu().double() * coef
                st = self.state.setdefault(id(p), {"m": torch.zeros_like(p), "v": torch.zeros_like(p), "t": 0})
                st["t"] += 1
                t = st["t"]
                p -= lr * wd * p
                st["m"] = st["m"] + (1.0 - BETA1) * (g - st["m"])
                st["v"] = BETA2 * st["v"] + (1.0 - BETA2) * g * g
                p -= (lr / (1.0 - BETA1 ** t)) * st["m"] / (st["v"].sqrt() / math.sqrt(1.0 - BETA2 ** t) + EPS)
        return norm, coef


# the optimizer test: fixed gradients scaled 1, 10, 0.1 from step to step; max_grad_norm = CLIP_FRACTION * (norm of the unscaled
# gradients), so the norms are N, 10 N, 0.1 N against 0.5 N: steps 1 and 2 clip, step 3 does not
STEP_SCALES = [1.0, 10.0, 0.1]
CLIP_FRACTION = 0.5
