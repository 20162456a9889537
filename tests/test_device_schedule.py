"""The schedule table behind AdamW(device_schedule=...), host side: its rows are the host's own per-step values bit
for bit, row t is update t of the loop `opt.step(); sched.step()`, the constructor refuses what one device counter cannot serve, and
the host mirror stops a step past the table's end.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from mtvaf_amd import optim
from mtvaf_amd.optim import AdamW, ScheduleMirror, ema_decay_at, linear_schedule_with_warmup, linear_warmup_factor, schedule_table

T, WARMUP, BETAS = 50, 4.5, (0.9, 0.999)  # (the reference passes a float warm-up count)


def _f32(x):
    """What a Python float becomes in a `float` argument of the C ABI."""
    return ctypes.c_float(x).value


def _params(n=2):
    return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]


@pytest.mark.parametrize("ema_warmup", [True, False])
def test_rows_are_the_hosts_own_values_bit_for_bit(ema_warmup):
    decay = 0.99
    table = schedule_table(linear_warmup_factor(WARMUP, T), T, BETAS, ema_decay=decay, ema_warmup=ema_warmup)
    assert len(table) == T == table.num_steps and table.rows.dtype.itemsize == 24
    assert table.rows.dtype.names == ("lr_factor", "bc1", "bc2_sqrt", "ema_omd", "pad")
    assert table.rows["lr_factor"].dtype == np.float64 and table.rows["bc1"].dtype == np.float32
    # the eager side: a LambdaLR on a stand-in optimizer, the bias corrections as mtvaf_amd.hip computes them, AdamW._ema_omd
    ref = torch.optim.SGD(_params(1), lr=1.0)
    sched = linear_schedule_with_warmup(ref, WARMUP, T)
    probe = AdamW(_params(1), ema_decay=decay, ema_warmup=ema_warmup)
    for t in range(1, T + 1):
        row = table.rows[t - 1]
        assert float(row["lr_factor"]) == ref.param_groups[0]["lr"], t  # (base lr 1: the factor itself, as a double)
        assert float(row["bc1"]) == _f32(float(1.0 - BETAS[0] ** t)), t
        assert float(row["bc2_sqrt"]) == _f32(float((1.0 - BETAS[1] ** t) ** 0.5)), t
        assert float(row["ema_omd"]) == _f32(probe._ema_omd(t - 1)) == _f32(1.0 - ema_decay_at(t - 1, decay, ema_warmup)), t
        assert int(row["pad"]) == 0
        ref.step()
        sched.step()
    assert table.lr_factors[T] == ref.param_groups[0]["lr"]  # what readers of group["lr"] see after the last update
    # the bytes the device reads: 24 per row, little-endian, in this order
    raw = table.rows.view(np.uint8).reshape(T, 24)
    assert raw[3, :8].tobytes() == np.float64(table.lr_factors[3]).tobytes()
    assert raw[3, 8:12].tobytes() == np.float32(1.0 - BETAS[0] ** 4).tobytes()


def test_row_t_holds_the_factor_of_update_t_in_the_eager_loop():
    """opt.step(); sched.step(): update t runs at base_lr * factor(t - 1) -- the scheduler's constructor applies factor(0), its t-th
    step() sets the lr of update t + 1.  Warm-up 4.5: the factor rises over updates 1 .. 5 and falls from update 6 on."""
    factor = linear_warmup_factor(WARMUP, T)
    table = schedule_table(factor, T, BETAS)
    opt = torch.optim.SGD(_params(1), lr=3e-3)
    sched = linear_schedule_with_warmup(opt, WARMUP, T)
    used = []
    for t in range(1, T + 1):
        used.append(opt.param_groups[0]["lr"])  # what this update's kernels are handed
        opt.step()
        sched.step()
    for t in range(1, T + 1):
        f = float(table.rows["lr_factor"][t - 1])
        assert f == factor(t - 1) and 3e-3 * f == used[t - 1], t
    f = table.rows["lr_factor"]
    assert f[0] == 0.0 and all(f[i] < f[i + 1] for i in range(4)) and f[5] > f[6] > f[7]
    assert f[1] == factor(1) != factor(2)  # (one off in either direction is another number)


def test_constructor_refusals():
    table = schedule_table(linear_warmup_factor(WARMUP, T), T, BETAS)
    a, b = _params(2)
    with pytest.raises(ValueError, match="betas"):
        AdamW([{"params": [a]}, {"params": [b], "betas": (0.8, 0.999)}], device_schedule=table)
    with pytest.raises(ValueError, match="overlap=False"):
        AdamW([a, b], overlap=True, device_schedule=table)
    short = schedule_table(linear_warmup_factor(WARMUP, T), T, BETAS)
    short.rows = short.rows[:T - 1]
    with pytest.raises(ValueError, match="fewer than"):
        AdamW([a, b], device_schedule=short)
    with pytest.raises(ValueError, match="ema_decay"):
        AdamW([a, b], ema_decay=0.9, device_schedule=table)  # (the table was built without an average)
    with pytest.raises(TypeError):
        AdamW([a, b], device_schedule=table.rows)
    with pytest.raises(ValueError):
        schedule_table(linear_warmup_factor(WARMUP, T), 0, BETAS)
    opt = AdamW([{"params": [a], "lr": 2e-3}, {"params": [b]}], lr=1e-3, device_schedule=table)
    assert [g["initial_lr"] for g in opt.param_groups] == [2e-3, 1e-3] and opt.schedule_count == 0


def test_host_mirror_raises_at_step_T_plus_1_and_the_mirror_scheduler_follows_the_table():
    factor = linear_warmup_factor(WARMUP, T)
    opt = AdamW(_params(2), lr=1e-3, device_schedule=schedule_table(factor, T, BETAS))
    sched = ScheduleMirror(opt)
    assert opt.param_groups[0]["lr"] == 1e-3 * factor(0)
    for t in range(1, T + 1):
        opt.host_step()  # (the bookkeeping of one update: no launch, so it runs here)
        with pytest.raises(AssertionError):
            opt.assert_schedule_agrees()  # the scheduler is one step behind
        sched.step()
        opt.assert_schedule_agrees()
        assert opt.schedule_count == t and opt.param_groups[0]["lr"] == 1e-3 * factor(t)
    with pytest.raises(RuntimeError, match="past the end"):
        opt.host_step()
    assert opt.schedule_count == T
    # a LambdaLR given the table's factor agrees as well
    opt2 = AdamW(_params(2), lr=1e-3, device_schedule=schedule_table(factor, T, BETAS))
    lam = torch.optim.lr_scheduler.LambdaLR(opt2, factor)
    opt2.assert_schedule_agrees()
    opt2.host_step()
    lam.step()
    opt2.assert_schedule_agrees()


def test_build_optimizer_leaves_the_default_alone():
    """args.device_schedule is off by default: the optimizer and scheduler types of the eager path (CPU: torch's own)."""
    import types
    m = torch.nn.Linear(4, 4)
    args = types.SimpleNamespace(lr=1e-3, use_prefix=False)
    opt, sched = optim.build_optimizer(m, args, 20)
    assert isinstance(opt, torch.optim.AdamW) and isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    args.device_schedule = True
    with pytest.raises(ValueError, match="device_schedule"):
        optim.build_optimizer(m, args, 20)
