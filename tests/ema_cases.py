"""Shared by test_ema.py (host) and test_ema_gpu.py: a float64 restatement of the exponential moving average the AdamW update
kernels keep (csrc/optim.hip, the *_ema entry points; mtvaf_amd.optim.AdamW(ema_decay=...)) and the case lists of the kernel tests.
No GPU, no library call.

The restatement: update number t (0-based) of an average uses the decay d_t = 0 for t == 0, min(decay, (1 + t) / (10 + t)) with
warm-up and `decay` without; the kernel receives omd = float32(1 - d_t) and does e <- e + omd * (p_new - e) on the parameter it has
just written.  The restatement is fed the kernel's own fp32 parameters of every step, so AdamW's rounding stays out of the
comparison, and the float32 omd the kernel was given, which is an input and not an error of its arithmetic.

The bound: one step rounds the difference p - e, then the fused product-and-sum -- two roundings of at most 2^-24 relative each, of
quantities no larger than 2 max(|p|, |e|) and max(|p|, |e|) -- and multiplies the error it inherited by d < 1.  After T steps
|e - e64| <= 2 T 2^-23 max(|p|, |e|), elementwise.

Which |p| and |e|: the difference that is rounded is p_new - e_OLD, and the inherited error is relative to the values of EARLIER
steps, so the magnitudes the derivation speaks of are those the recurrence has passed through -- `Ema64.mag`, the running elementwise
maximum of |p_s| and |e_s| over the steps so far, the average that entered a step included.  Read with the values of the last step
alone the inequality cannot hold for any evaluation of the prescribed fmaf, correctly rounded as it is, in an element whose
parameter crosses zero: Adam moves a parameter by about lr per step whatever its size, so in a 77 k-element table a few elements
have |p_new| and |e_new| far below |p_new - e_old|, whose rounding then exceeds that reading (measured on the tiny encoder, lr 1e-3,
second step: 1.05 of it; with the running maximum: 0.2).  `Ema64.worst_last_values` still reports that figure."""
import numpy as np
import torch

# lengths at which the update bodies switch: below / at / above one float4, a scalar tail behind several float4 rows, and more
# than one 256-lane block's 1024 elements ... up to more than 64 blocks with a tail
LENGTHS = [1, 3, 4, 5, 1027, 65536 + 4]
# which buffers start 4 bytes behind a 16-byte boundary (the scalar body): none, only the average, only the parameter
ALIGNMENTS = {"aligned": (), "ema_offset": ("e",), "p_offset": ("p",)}
MAX_BLOCKS = [0, 1]
STEPS = 6            # one step at omd = 1, five at omd = 0.1
OMD_FIRST, OMD = 1.0, 0.1
HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2)  # lr, beta1, beta2, eps, weight decay

# the multi-tensor form: 49 tensors, one more than a launch takes; lengths mixed, 1 included
MULTI_LENGTHS = LENGTHS + [7 + 13 * i for i in range(43)]
assert len(MULTI_LENGTHS) == 49

# the planes form: four of the smallest legal matrices (cols = 32; rows 4 and 8) in one flat buffer, with stretches that belong to
# no matrix between and behind them.  (first element, rows, cols); every begin and the total are multiples of 4
PLANE_SEGS = [(0, 4, 32), (140, 8, 32), (404, 4, 32), (544, 8, 32)]
PLANE_N = 820
assert all(b % 4 == 0 for b, _, _ in PLANE_SEGS) and PLANE_N % 4 == 0
assert all(PLANE_SEGS[i][0] + PLANE_SEGS[i][1] * PLANE_SEGS[i][2] < PLANE_SEGS[i + 1][0] for i in range(3))
assert PLANE_SEGS[3][0] + PLANE_SEGS[3][1] * PLANE_SEGS[3][2] < PLANE_N


def decay_at(t: int, decay: float, warmup: bool) -> float:
    if t == 0:
        return 0.0
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def as_f32(x: float) -> float:
    """x rounded to float: a scalar as the kernel receives it."""
    return float(np.float32(x))


def omd32(d: float) -> float:
    """1 - d rounded once from double to float: what crosses the C ABI."""
    return float(np.float32(1.0 - d))


def ema64_step(e64: torch.Tensor, p: torch.Tensor, omd: float) -> torch.Tensor:
    """e64 (float64) after one more parameter p (the kernel's fp32 values), omd already a float32 value."""
    return e64 + omd * (p.detach().cpu().double() - e64)


def bound(T: int, p: torch.Tensor, e64: torch.Tensor) -> torch.Tensor:
    return 2.0 * T * 2.0 ** -23 * torch.maximum(p.detach().cpu().double().abs(), e64.abs())


def worst(e: torch.Tensor, e64: torch.Tensor, T: int, p: torch.Tensor) -> float:
    """max |e - e64| in units of the bound (<= 1 passes); 0 where the bound is 0 and the error too."""
    err = (e.detach().cpu().double() - e64).abs()
    b = bound(T, p, e64)
    ok_zero = (b == 0) & (err == 0)
    ratio = torch.where(ok_zero, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


class Ema64:
    """The float64 average of one tensor and the magnitudes its bound is relative to."""

    def __init__(self, like: torch.Tensor):
        self.e = torch.zeros(like.shape, dtype=torch.float64)
        self.mag = torch.zeros(like.shape, dtype=torch.float64)
        self.T = 0
        self.p = None

    def step(self, p: torch.Tensor, omd: float):
        """One more update with the kernel's fp32 parameter p; omd already a float32 value."""
        self.p = p.detach().cpu().double()
        self.mag = torch.maximum(self.mag, torch.maximum(self.p.abs(), self.e.abs()))
        self.e = self.e + omd * (self.p - self.e)
        self.mag = torch.maximum(self.mag, self.e.abs())
        self.T += 1
        return self

    def _ratio(self, e, mag):
        err = (e.detach().cpu().double() - self.e).abs()
        b = 2.0 * self.T * 2.0 ** -23 * mag
        r = torch.where((b == 0) & (err == 0), torch.zeros_like(err), err / b.clamp_min(1e-300))
        return float(r.max()) if r.numel() else 0.0

    def worst(self, e: torch.Tensor) -> float:
        """max |e - e64| in units of 2 T 2^-23 mag (<= 1 passes)."""
        return self._ratio(e, self.mag)

    def worst_last_values(self, e: torch.Tensor) -> float:
        """The same in units of 2 T 2^-23 max(|p|, |e|) of the last step alone (reported, see the head of this file)."""
        return self._ratio(e, torch.maximum(self.p.abs(), self.e.abs()))


def step_omds():
    return [OMD_FIRST] + [OMD] * (STEPS - 1)
