"""The averaged weights (EMA) of mtvaf_amd.optim.AdamW, host side: the decay schedule, the constructor's validation, the entry
points the library exports, and the float64 restatement the GPU tests measure against."""
import math
import types

import pytest
import torch

import ema_cases as EC

NEW_SYMBOLS = ["mtvaf_adamw_ema", "mtvaf_adamw_planes_ema", "mtvaf_adamw_multi_ema", "mtvaf_swap_f32_multi"]


@pytest.mark.parametrize("t, decay, warmup, want", [
    (0, 0.999, True, 0.0), (0, 0.9, False, 0.0), (0, 0.5, True, 0.0),
    (1, 0.999, True, 2.0 / 11.0),
    (89, 0.9, True, 0.9),
    (90, 0.9, True, 0.9),
    (5, 0.9, False, 0.9),
])
def test_ema_decay_at(t, decay, warmup, want):
    from mtvaf_amd.optim import ema_decay_at
    got = ema_decay_at(t, decay, warmup)
    assert got == want and isinstance(got, float)
    assert got == EC.decay_at(t, decay, warmup)  # the restatement the GPU tests use follows the same rule


def test_warmup_never_exceeds_the_decay_and_reaches_it():
    from mtvaf_amd.optim import ema_decay_at
    ds = [ema_decay_at(t, 0.999, True) for t in range(20000)]
    assert ds[0] == 0.0 and all(a <= b for a, b in zip(ds, ds[1:])) and max(ds) == 0.999 == ds[-1]
    assert ds[1:4] == [2.0 / 11.0, 3.0 / 12.0, 4.0 / 13.0]


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan")])
def test_constructor_refuses_a_decay_outside_the_half_open_unit_interval(bad):
    from mtvaf_amd.optim import AdamW
    with pytest.raises(ValueError, match="ema_decay"):
        AdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, ema_decay=bad)


def test_constructor_with_a_decay_touches_nothing():
    """CPU parameters, no library call, no state: the averages are created by the first update."""
    from mtvaf_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.ones(2, 3))]
    opt = AdamW(p, lr=1e-3, ema_decay=0.9)
    assert opt.ema_decay == 0.9 and opt.ema_warmup is True and opt.ema_swapped is False
    assert len(opt.state) == 0 and "ema_decay" not in opt.defaults and all("ema_decay" not in g for g in opt.param_groups)
    assert "ema_decay: 0.9" in repr(opt)
    off = AdamW(p, lr=1e-3)
    assert off.ema_decay == 0.0 and "ema_decay" not in repr(off)
    assert AdamW(p, lr=1e-3, ema_decay=0.5, ema_warmup=False).ema_warmup is False
    with pytest.raises(RuntimeError, match="ema_decay == 0"):
        off.swap_ema()


def test_build_optimizer_on_a_cpu_model_refuses_to_ignore_ema_decay():
    """As for max_grad_norm: the CPU fallback is torch.optim.AdamW, which keeps no average."""
    from mtvaf_amd.optim import build_optimizer
    model = torch.nn.Linear(4, 3)
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=False, ema_decay=0.99)
    with pytest.raises(ValueError, match="ema_decay"):
        build_optimizer(model, args, 10)
    args.ema_decay = 0.0
    opt, _ = build_optimizer(model, args, 10)
    assert isinstance(opt, torch.optim.AdamW)


def test_library_exports_the_ema_entry_points():
    from mtvaf_amd import hip
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    hip.lib()  # binds them: raises if the built library lacks one


def test_restatement_and_bound():
    """omd = 1 on a zero average gives the parameter exactly; a constant parameter is a fixed point; the recurrence is the closed
    form; the bound is elementwise and scales with the step count."""
    p = torch.tensor([1.5, -2.0, 0.0, 3e-8], dtype=torch.float32)
    e = EC.ema64_step(torch.zeros(4, dtype=torch.float64), p, 1.0)
    assert torch.equal(e, p.double())
    assert torch.equal(EC.ema64_step(e, p, EC.omd32(0.9)), e)
    q = torch.tensor([2.5, -1.0, 1.0, 0.0], dtype=torch.float32)
    o = EC.omd32(0.9)
    assert abs(o - 0.1) < 2.0 ** -27 and o != 0.1  # rounded once to float, not the double
    e2 = EC.ema64_step(e, q, o)
    torch.testing.assert_close(e2, (1.0 - o) * p.double() + o * q.double(), rtol=1e-15, atol=0)
    b = EC.bound(3, q, e2)
    assert torch.equal(b, 6.0 * 2.0 ** -23 * torch.maximum(q.double().abs(), e2.abs()))
    assert EC.worst(e2.float(), e2, 1, q) <= 0.5 + 1e-9  # one rounding to float is a quarter of the one-step bound at most
    assert EC.worst((e2 * (1 + 2.0 ** -20)).float(), e2, 1, q) > 1.0
    assert EC.step_omds() == [1.0, 0.1, 0.1, 0.1, 0.1, 0.1] and len(EC.MULTI_LENGTHS) == 49 and 1 in EC.MULTI_LENGTHS
    assert math.isclose(EC.decay_at(1, 0.999, True), 2.0 / 11.0)


def test_bound_is_relative_to_the_magnitudes_the_recurrence_passed_through():
    """An element whose parameter crosses zero: the fp32 evaluation of the prescribed fmaf, every operation correctly rounded, stays
    inside the bound over the running maximum -- and can exceed the same expression over the last step's values alone, which is
    why the GPU tests assert the former and print the latter."""
    import numpy as np
    g = torch.Generator().manual_seed(0)
    n = 200000
    p0 = (torch.randn(n, generator=g) * 2e-3).float()
    # an Adam-sized step whatever the magnitude, behind a weight decay: p1 - p0 is not an exact float
    x = 1e-3 * (1.0 + 0.3 * torch.rand(n, generator=g)) * torch.sign(torch.randn(n, generator=g))
    p1 = (p0.double() * (1.0 - 1e-5) - x.double() * 1.0000001).float()
    omd = EC.omd32(EC.decay_at(1, 0.9, True))
    ref = EC.Ema64(p0).step(p0, 1.0)
    e = p0.clone()  # fmaf(1, p - 0, 0)
    assert ref.worst(e) == 0.0
    ref.step(p1, omd)
    d = (p1 - e)  # fp32, rounded once
    e1 = torch.from_numpy(np.float32(e.double().numpy() + np.float64(omd) * d.double().numpy()))  # the fma: one more rounding
    assert ref.T == 2 and ref.worst(e1) <= 0.5
    print(ref.worst(e1), ref.worst_last_values(e1))
    assert ref.worst_last_values(e1) > 1.0  # (about 1.14 at most: p1 = -e1 = 0.09 |p1 - p0| and a half-ulp rounding of the difference)
