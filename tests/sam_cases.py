"""Case table, input builders and the plain float64 restatement of the contract of mtvaf_sam_finalize / mtvaf_sam_perturb
(include/mtvaf_hip.h, csrc/gradnorm.hip, csrc/optim.hip).  Shared by test_sam_cases.py (CPU: proves the restatement against a
textbook SAM loop) and test_sam_gpu.py (the kernels, AdamW.perturb / step, SharpnessAware).  Nothing here imports mtvaf_amd: torch and
numpy on the host, float64 from the fp32 inputs.

The bounds, derived from the arithmetic (nothing below is fitted to an output):

  * the sum of squares is formed in double from the first operation (relative error n 2^-53, nothing beside an fp32 ulp), the norm
    is its square root rounded ONCE to fp32: within 1 fp32 ulp of the float64 norm (half an ulp from the rounding, the rest head-room
    for the host summing the squares in another order).
  * scale = (float)(rho / (norm64 + 1e-12)) with norm64 = sqrt(sum of the device's own partials in index order): IEEE double
    addition, sqrt and division are correctly rounded on both sides, so the host reproduces the bits -- compared exactly.
  * p_new = fmaf(scale, g, p) is one correctly rounded operation: |p_new - (p + scale g)| <= 0.5 ulp32(p_new), the exact value
    evaluated in float64 (product exact in 48 bits, the sum's error 2^-53 relative: 2^-29 of that half-ulp)."""
import math

import numpy as np
import torch

RHO = 0.05
CHUNK = 65536                                   # elements per partial sum of mtvaf_grad_sqnorm_multi
SIZES = (1, 3, 4, 5, 65532, 65536, 65540)       # scalar tail only, one float4, the chunk edge of the norm from both sides
# (length, elements the base is moved off a 16-byte boundary): every size, some bases 4 bytes off
MULTI = tuple((n, 1 if i % 2 else 0) for i, n in enumerate(SIZES)) + ((65540, 1), (7, 0))
KINDS = ("randn", "scaled-down", "scaled-up", "zero", "overflow32", "inf", "nan")


def _case(n, kind):
    return dict(id=f"n{n}-{kind}", n=n, kind=kind)


CASES = [_case(n, "randn") for n in SIZES] + [_case(65540, k) for k in KINDS[1:]] + [_case(5, k) for k in KINDS[1:]]


def make_inputs(n, kind="randn", seed=0):
    """-> p, g fp32 [n] on the host.  scaled-down / scaled-up: g * 2^-60 / 2^+60 (the norm is finite in double and in fp32);
    overflow32: every element 3e38, so that the norm (3e38 sqrt(n)) is finite in double and not in fp32 for n >= 2;
    inf / nan: one such element in the middle."""
    gen = torch.Generator().manual_seed(2000 + seed + n)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 1e-2
    if kind == "scaled-down":
        g = g * 2.0 ** -60
    elif kind == "scaled-up":
        g = g * 2.0 ** 60
    elif kind == "zero":
        g = torch.zeros(n)
    elif kind == "overflow32":
        g = torch.full((n,), 3e38)
    elif kind == "inf":
        g[n // 2] = float("inf")
    elif kind == "nan":
        g[n // 2] = float("nan")
    return p, g


def ordered_norm64(partials):
    """sqrt of the partial sums added in index order, in double: what the finalize kernel computes."""
    s = 0.0
    for x in partials:
        s += float(x)
    return math.sqrt(s)


def host_partials(gs):
    """The partial sums of mtvaf_grad_sqnorm_multi over these tensors (one per 65536-element chunk, tensor after tensor), float64
    on the host -- each chunk summed in whatever order torch takes."""
    out = []
    for g in gs:
        g64 = g.double().reshape(-1)
        out.extend(float((c * c).sum()) for c in g64.split(CHUNK))
    return out


def scale32(rho, norm64):
    """(float)((double)(float)rho / (norm64 + 1e-12)) -> numpy float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float64(np.float32(rho)) / (np.float64(norm64) + np.float64(1e-12)))


def fits32(norm64):
    with np.errstate(over="ignore", invalid="ignore"):
        n32 = np.float32(norm64)
    return bool(np.isfinite(n32))


def reference(ps, gs, rho, scale=None):
    """The contract in float64 over lists of tensors: -> dict norm (float64 global norm), finite (the norm fits fp32), scale (the one
    given -- the kernel's own fp32 value -- or rho / (norm + 1e-12) in double), p_new (list, float64: p + scale g, or p where not
    finite)."""
    norm = ordered_norm64(host_partials(gs))
    finite = fits32(norm)
    if scale is None:
        scale = float(np.float32(rho)) / (norm + 1e-12) if finite else 0.0
    new = [p.double() + float(scale) * g.double() if finite else p.double() for p, g in zip(ps, gs)]
    return dict(norm=norm, finite=finite, scale=float(scale), p_new=new)


def ulp32(x):
    """spacing of fp32 at |x| (float64 tensor in, float64 out); the smallest subnormal at 0"""
    a = x.abs().float()
    up = torch.nextafter(a, torch.full_like(a, float("inf")))
    return (up.double() - a.double())


def half_ulp_excess(p_new, exact):
    """max |p_new - exact| / (0.5 ulp32(p_new)) over the elements; inf if p_new holds a non-finite value"""
    got = p_new.detach().double().cpu().reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    q = (got - exact.reshape(-1)).abs() / (0.5 * ulp32(got))
    return float(q.max()) if q.numel() else 0.0
