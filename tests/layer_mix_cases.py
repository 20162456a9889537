"""Case table, input builders and the float64 reference of the layer mix (csrc/layermix.hip; include/mtvaf_hip.h:
mtvaf_layer_mix_fwd / _dots / _inject).  Shared by test_layer_mix.py (CPU: the reference's analytic
gradients against finite differences of itself) and test_layer_mix_gpu.py (the kernels).  Nothing here imports mtvaf_amd: torch on
the host only.

    y = gamma * sum_j s_j h_j,  s = softmax(a);   with t_j = sum dy * h_j:
    d gamma = sum_j s_j t_j,   d a_j = gamma s_j (t_j - sum_i s_i t_i),   d h_j = gamma s_j dy

The tolerance of a kernel result is not a constant: it is FACTOR times the error the same formula has as an fp32 eager torch chain
on the host (stack, softmax, weighted sum, autograd) against the float64 reference -- `bound`.  The error of ONE element of that
chain is an accident of rounding (any fraction of an ulp, 0 included), so it is taken as the maximum over the elements of one
magnitude class: the columns the inputs scale by 1e-12, those they scale by 1e+6 and the rest, each over all rows (for the [K]
vectors: over the vector).  Where that maximum is 0 -- a chain that happens to be exact, K = 1 or gamma = 0 -- ULPS ulps of the
class's largest reference value."""
import functools

import torch

# (K, rows, H, scalars, gamma): every K of {1, 2, 13, 25, 32}, every row count of {1, 63, 64, 65, 257}, every H of {64, 768, 1024}, the
# three scalar patterns and every gamma of {1, -0.5, 0} occur; rows 63 / 65 / 257 leave partial blocks, 257 x 1024 needs more than one
# block per state in every kernel and a grid-stride loop in none -- 1031 rows of H = 1024 does (more float4 groups than 1024 blocks
# x 256 threads hold)
CASES = [
    (1, 1, 64, "equal", 1.0),
    (2, 63, 64, "pm80", -0.5),
    (13, 64, 768, "random", 1.0),
    (13, 65, 768, "equal", -0.5),
    (25, 257, 64, "pm80", 1.0),
    (32, 257, 1024, "random", -0.5),
    (32, 65, 768, "pm80", 0.0),
    (2, 257, 1024, "equal", 0.0),
    (13, 1, 1024, "pm80", 1.0),
    (25, 63, 768, "random", 0.0),
    (32, 64, 64, "equal", 1.0),
    (1, 257, 768, "random", -0.5),
    (2, 1031, 1024, "random", 1.0),
]
IDS = [f"K{k}-r{r}-H{h}-{s}-g{g}" for k, r, h, s, g in CASES]
FACTOR = 4.0  # kernel error <= FACTOR x the eager chain's: fmaf against separate multiply-add, another expf
ULPS = 4.0    # where the eager chain is exact
SMALL, LARGE = 1e-12, 1e6


def column_scale(H):
    """[H]: one column in eight scaled by 1e-12, one in eight by 1e+6."""
    c = torch.arange(H)
    scale = torch.ones(H, dtype=torch.float32)
    scale[c % 8 == 1] = SMALL
    scale[c % 8 == 5] = LARGE
    return scale


def column_class(H):
    """[H] int: 0 ordinary, 1 the 1e-12 columns, 2 the 1e+6 columns."""
    c = torch.arange(H)
    cls = torch.zeros(H, dtype=torch.long)
    cls[c % 8 == 1] = 1
    cls[c % 8 == 5] = 2
    return cls


def make_scalars(K, pattern, gen):
    if pattern == "equal":
        return torch.full((K,), 0.25, dtype=torch.float32)
    a = torch.randn(K, generator=gen, dtype=torch.float32)
    if pattern == "pm80":  # the largest first, the smallest last; K = 1: the one value is +80
        a[0] = 80.0
        if K > 1:
            a[-1] = -80.0
    else:
        assert pattern == "random", pattern
    return a


@functools.lru_cache(maxsize=None)
def make_inputs(i):
    """-> (states [K,rows,H], dy [rows,H], scalars [K], gamma [1]) of case i, fp32 on the host.  Built once, never written to."""
    K, rows, H, pattern, gamma = CASES[i]
    gen = torch.Generator().manual_seed(1000 + i)
    scale = column_scale(H)
    states = torch.randn(K, rows, H, generator=gen, dtype=torch.float32) * scale
    dy = torch.randn(rows, H, generator=gen, dtype=torch.float32) * scale
    return states, dy, make_scalars(K, pattern, gen), torch.tensor([gamma], dtype=torch.float32)


def reference(states, dy, scalars, gamma):
    """The float64 reference -> dict(s, y, t, dgamma, dscalars, coef); dh_j = coef[j] * dy.  d scalars in the form
    gamma s_j sum_i s_i (t_j - t_i), which equals gamma s_j (t_j - sum_i s_i t_i) for weights that add up to 1 and does not cancel
    where one weight is (nearly) 1."""
    h, d, a, g = states.double(), dy.double(), scalars.double(), gamma.double().reshape(())
    s = torch.softmax(a, 0)
    y = g * torch.einsum("j,jrc->rc", s, h)
    t = torch.einsum("rc,jrc->j", d, h)
    dgamma = (s * t).sum()
    dscalars = g * s * ((t[:, None] - t[None, :]) * s[None, :]).sum(1)
    return dict(s=s, y=y, t=t, dgamma=dgamma.reshape(1), dscalars=dscalars, coef=g * s)


def forward64(states, scalars, gamma):
    """y alone, differentiable: what the finite differences of test_layer_mix.py step."""
    return gamma.reshape(()) * torch.einsum("j,jrc->rc", torch.softmax(scalars, 0), states)


def eager32(states, dy, scalars, gamma):
    """The same formula as an fp32 eager torch chain with autograd, on the host -> dict(y, dgamma, dscalars, dh [K,rows,H])."""
    hs = [h.clone().requires_grad_(True) for h in states]
    a, g = scalars.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    s = torch.softmax(a, 0)
    y = g * (torch.stack(hs) * s.view(-1, 1, 1)).sum(0)
    y.backward(dy)
    return dict(y=y.detach(), dgamma=g.grad, dscalars=a.grad, dh=torch.stack([h.grad for h in hs]))


def ulp32(x):
    """Spacing of fp32 at |x| (float64 in, float64 out)."""
    x = x.abs().float().clamp_min(torch.finfo(torch.float32).tiny)
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _class_bound(err, ref, cls):
    """Per element: FACTOR x the largest eager error of the element's class, or ULPS ulps of the class's largest |ref| where that
    error is 0.  err, ref [..., H] float64; cls [H]."""
    out = torch.empty_like(err)
    for c in range(3):
        sel = cls == c
        if not bool(sel.any()):
            continue
        e = float(err[..., sel].max())
        out[..., sel] = FACTOR * e if e > 0 else ULPS * float(ulp32(ref[..., sel].abs().max()))
    return out


def _vector_bound(err, ref):
    e = float(err.max())
    return torch.full_like(err, FACTOR * e if e > 0 else ULPS * float(ulp32(ref.abs().max())))


@functools.lru_cache(maxsize=None)
def bounds(i):
    """-> (reference dict, bound dict over y, dgamma, dscalars, dh) of case i; computed once."""
    states, dy, scalars, gamma = make_inputs(i)
    ref = reference(states, dy, scalars, gamma)
    eag = eager32(states, dy, scalars, gamma)
    cls = column_class(states.shape[2])
    dh64 = ref["coef"].view(-1, 1, 1) * dy.double()
    bound = dict(y=_class_bound((eag["y"].double() - ref["y"]).abs(), ref["y"], cls),
                 dh=_class_bound((eag["dh"].double() - dh64).abs(), dh64, cls),
                 dgamma=_vector_bound((eag["dgamma"].double() - ref["dgamma"]).abs(), ref["dgamma"]),
                 dscalars=_vector_bound((eag["dscalars"].double() - ref["dscalars"]).abs(), ref["dscalars"]))
    return dict(ref, dh=dh64), bound


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound: <= 1 passes.  (bound 0 and error 0: 0.)"""
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max())


def resolve_reference(layers, n):
    """What `engine.resolve_mix_layers` documents, restated: -> sorted tuple, or ValueError."""
    if layers == "all":
        idx = list(range(n))
    else:
        idx = []
        for k in layers:
            if not -n <= k < n:
                raise ValueError(k)
            idx.append(k % n)
        if len(set(idx)) != len(idx):
            raise ValueError("duplicate")
    if not 1 <= len(idx) <= 32:
        raise ValueError(len(idx))
    return tuple(sorted(idx))
