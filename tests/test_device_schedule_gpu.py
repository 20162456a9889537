"""The step's hyper-parameters on the device: every *_sched update kernel against today's entry point fed the host's
per-step floats, bit for bit; the device guard past the table's end; AdamW(device_schedule=...) against AdamW + LambdaLR, eagerly and
through a state_dict round trip; and the whole training step, optimizer included, replayed from one captured graph."""
import copy
import itertools

import pytest
import torch

from test_adamw_segments_gpu import TINY, _batch, _compute, _model
from test_model_gpu import DEV

import params as P

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
STEPS, ROWS = 6, 8
DECAY = 0.99
COEF = 0.37  # of the clip state: a gradient scale that is not a power of two


def _factor():
    from mtvaf_amd.optim import linear_warmup_factor
    return linear_warmup_factor(2.5, 20)  # rises over updates 1 .. 3, falls from update 4 on: both inside the 6 steps


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Sched:
    """The table on the device, the counter and the 32-byte block."""

    def __init__(self, rows=ROWS, factor=None):
        import numpy as np
        from mtvaf_amd.optim import schedule_table
        self.host = schedule_table(factor or _factor(), rows, (B1, B2), ema_decay=DECAY)
        self.table = torch.from_numpy(self.host.rows.view(np.uint8).copy()).to(DEV)
        self.counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.current = torch.zeros(4, dtype=torch.int64, device=DEV)

    def advance(self):
        from mtvaf_amd import hip
        hip.adamw_sched_advance(self.table, self.counter, self.current)


def _host_step(t):
    """(lr factor, 1 - decay) the eager loop hands update t (1-based)."""
    from mtvaf_amd.optim import ema_decay_at
    return _factor()(t - 1), float(1.0 - ema_decay_at(t - 1, DECAY, True))


def _case(n, seed, off=0):
    """p, m, v, an average, a bf16 shadow and STEPS gradients of n elements on the device; off: every fp32 base `off` floats past a
    16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda x: torch.cat([torch.zeros(off), x]).to(DEV)[off:]
    p, m, v = mk(torch.randn(n, generator=g)), mk(torch.randn(n, generator=g) * 0.01), mk(torch.rand(n, generator=g) * 0.01)
    e = mk(torch.randn(n, generator=g))
    sh = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
    grads = [mk(torch.randn(n, generator=g) * 0.1) for _ in range(STEPS)]
    return dict(p=p, m=m, v=v, e=e, sh=sh, grads=grads)


def _clip():
    return torch.tensor([1.0, COEF, 1.0, 0.0], device=DEV)


def _opts(clip, ema, shadow, c, host_omd=None):
    kw = {}
    if clip:
        kw["clip"] = _clip()
    if ema:
        kw["ema"] = c["e"]
        if host_omd is not None:
            kw["ema_omd"] = host_omd
    if shadow:
        kw["p_bf16"] = c["sh"]
    return kw


def _assert_same_case(a, b, what):
    for k in ("p", "m", "v", "e", "sh"):
        assert _equal(a[k], b[k]), (what, k)


N_FLAT = 4 * 257 + 3  # a vector body of 257 float4s (two blocks) and a scalar tail of 3
ALL8 = list(itertools.product((False, True), repeat=3))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4bytes"])
@pytest.mark.parametrize("clip,ema,shadow", ALL8)
def test_flat_update_on_the_device_schedule_has_the_bits_of_the_host_fed_update(clip, ema, shadow, off):
    from mtvaf_amd import hip
    a, b = _case(N_FLAT, 1, off), _case(N_FLAT, 1, off)
    assert a["p"].data_ptr() % 16 == 4 * off
    s = _Sched()
    lr, wd = 3e-3, 1e-2
    for t in range(1, STEPS + 1):
        f, omd = _host_step(t)
        hip.adamw(a["p"], a["grads"][t - 1], a["m"], a["v"], lr * f, B1, B2, EPS, wd, t, **_opts(clip, ema, shadow, a, omd))
        s.advance()
        hip.adamw_sched(b["p"], b["grads"][t - 1], b["m"], b["v"], lr, B1, B2, EPS, wd, s.current, **_opts(clip, ema, shadow, b))
        _assert_same_case(a, b, t)
    assert int(s.counter) == STEPS and not _equal(a["p"], _case(N_FLAT, 1, off)["p"])


SEGS = [(512, 1e-3, 1e-2), (1028, 2.5e-3, 0.0), (1029, 7e-4, 3e-2)]  # the last segment: ONE element, the scalar tail (n % 4 == 1)


@pytest.mark.parametrize("clip,ema,shadow", ALL8)
def test_segmented_update_on_the_device_schedule(clip, ema, shadow):
    from mtvaf_amd import hip
    n = SEGS[-1][0]
    a, b = _case(n, 2), _case(n, 2)
    s = _Sched()
    for t in range(1, STEPS + 1):
        f, omd = _host_step(t)
        hip.adamw_seg(a["p"], a["grads"][t - 1], a["m"], a["v"], [(e, lr * f, wd) for e, lr, wd in SEGS], B1, B2, EPS, t,
                      **_opts(clip, ema, shadow, a, omd))
        s.advance()
        hip.adamw_seg_sched(b["p"], b["grads"][t - 1], b["m"], b["v"], SEGS, B1, B2, EPS, s.current, **_opts(clip, ema, shadow, b))
        _assert_same_case(a, b, t)


MATS = [(0, 32, 64), (32 * 64 + 64, 64, 32)]  # one 32 x 64 and one 64 x 32 matrix, 64 loose elements between and behind them
PLANE_N = 32 * 64 + 64 + 64 * 32 + 64
PLANE_SEGS = [(2048, 1e-3, 1e-2), (2052, 2.5e-3, 0.0), (PLANE_N, 7e-4, 3e-2)]  # (n % 4 == 0 here: the short segment is one float4)


def _images():
    return [(b, r, c, torch.full((6 * r * c,), 0x7f, dtype=torch.uint8, device=DEV)) for b, r, c in MATS]


@pytest.mark.parametrize("segmented", [False, True], ids=["planes", "planes_seg"])
@pytest.mark.parametrize("clip,ema", list(itertools.product((False, True), repeat=2)))
def test_plane_image_updates_on_the_device_schedule(clip, ema, segmented):
    from mtvaf_amd import hip
    a, b = _case(PLANE_N, 3), _case(PLANE_N, 3)
    ia, ib = _images(), _images()
    s = _Sched()
    lr, wd = 3e-3, 1e-2
    for t in range(1, STEPS + 1):
        f, omd = _host_step(t)
        ka, kb = _opts(clip, ema, False, a, omd), _opts(clip, ema, False, b)
        s.advance()
        if segmented:
            hip.adamw_planes_seg(a["p"], a["grads"][t - 1], a["m"], a["v"], [(e, l * f, w) for e, l, w in PLANE_SEGS], B1, B2, EPS, t, ia,
                                 **ka)
            hip.adamw_planes_seg_sched(b["p"], b["grads"][t - 1], b["m"], b["v"], PLANE_SEGS, B1, B2, EPS, s.current, ib, **kb)
        else:
            hip.adamw_planes(a["p"], a["grads"][t - 1], a["m"], a["v"], lr * f, B1, B2, EPS, wd, t, ia, **ka)
            hip.adamw_planes_sched(b["p"], b["grads"][t - 1], b["m"], b["v"], lr, B1, B2, EPS, wd, s.current, ib, **kb)
        _assert_same_case(a, b, t)
        for x, y in zip(ia, ib):
            assert torch.equal(x[3], y[3]), t
    assert not bool((ib[0][3] == 0x7f).all())


def _multi_case(seed):
    """49 tensors (one launch of 48 and one of 1): lengths 1 .. 48 and one of N_FLAT, every third one 4 bytes off a 16-byte base."""
    return [_case(N_FLAT if i == 48 else i + 1, seed + i, off=1 if i % 3 == 0 else 0) for i in range(49)]


@pytest.mark.parametrize("clip,ema", list(itertools.product((False, True), repeat=2)))
def test_multi_tensor_update_on_the_device_schedule_across_the_48_tensor_split(clip, ema):
    from mtvaf_amd import hip
    a, b = _multi_case(100), _multi_case(100)
    s = _Sched()
    lr, wd = 3e-3, 1e-2
    col = lambda cs, k: [c[k] for c in cs]
    for t in range(1, STEPS + 1):
        f, omd = _host_step(t)
        ka = dict(clip=_clip() if clip else None, **(dict(ema=col(a, "e"), ema_omd=omd) if ema else {}))
        kb = dict(clip=_clip() if clip else None, ema=col(b, "e") if ema else None)
        hip.adamw_multi(col(a, "p"), [c["grads"][t - 1] for c in a], col(a, "m"), col(a, "v"), lr * f, B1, B2, EPS, wd, t, **ka)
        s.advance()
        hip.adamw_multi_sched(col(b, "p"), [c["grads"][t - 1] for c in b], col(b, "m"), col(b, "v"), lr, B1, B2, EPS, wd, s.current, **kb)
    for i, (x, y) in enumerate(zip(a, b)):
        _assert_same_case(x, y, i)
    assert not _equal(a[48]["p"], _multi_case(100)[48]["p"])


def test_past_the_end_of_the_table_the_flag_is_set_and_every_update_writes_nothing():
    """Through hip.py alone (the optimizer's host mirror would have raised first): a 3-row table, the 4th advance."""
    from mtvaf_amd import hip
    s = _Sched(rows=3)
    for t in range(1, 4):
        s.advance()
        cur = s.current.cpu()
        assert int(s.counter) == t == int(cur[3]) and int(cur.view(torch.int32)[5]) == 0
        assert float(cur.view(torch.float64)[0]) == s.host.lr_factors[t - 1]
        assert cur.view(torch.float32)[2:5].tolist() == [float(s.host.rows[k][t - 1]) for k in ("bc1", "bc2_sqrt", "ema_omd")]
    s.advance()
    cur = s.current.cpu()
    assert int(s.counter) == 4 == int(cur[3]) and int(cur.view(torch.int32)[5]) == 1
    assert float(cur.view(torch.float64)[0]) == s.host.lr_factors[2]  # (the last row: the index is clamped)
    lr, wd = 3e-3, 1e-2
    c, keep = _case(N_FLAT, 7), _case(N_FLAT, 7)
    hip.adamw_sched(c["p"], c["grads"][0], c["m"], c["v"], lr, B1, B2, EPS, wd, s.current, clip=_clip(), ema=c["e"], p_bf16=c["sh"])
    _assert_same_case(c, keep, "flat")
    c, keep = _case(SEGS[-1][0], 8), _case(SEGS[-1][0], 8)
    hip.adamw_seg_sched(c["p"], c["grads"][0], c["m"], c["v"], SEGS, B1, B2, EPS, s.current, ema=c["e"], p_bf16=c["sh"])
    _assert_same_case(c, keep, "seg")
    for segmented in (False, True):
        c, keep, imgs = _case(PLANE_N, 9), _case(PLANE_N, 9), _images()
        if segmented:
            hip.adamw_planes_seg_sched(c["p"], c["grads"][0], c["m"], c["v"], PLANE_SEGS, B1, B2, EPS, s.current, imgs, ema=c["e"])
        else:
            hip.adamw_planes_sched(c["p"], c["grads"][0], c["m"], c["v"], lr, B1, B2, EPS, wd, s.current, imgs, ema=c["e"])
        _assert_same_case(c, keep, "planes")
        assert all(bool((i[3] == 0x7f).all()) for i in imgs)
    cs, keeps = _multi_case(200), _multi_case(200)
    hip.adamw_multi_sched([x["p"] for x in cs], [x["grads"][0] for x in cs], [x["m"] for x in cs], [x["v"] for x in cs], lr, B1, B2, EPS,
                          wd, s.current, ema=[x["e"] for x in cs])
    for i, (x, y) in enumerate(zip(cs, keeps)):
        _assert_same_case(x, y, ("multi", i))
    # and with the counter back inside the table the same launch writes again
    s.counter.fill_(1)
    s.advance()
    hip.adamw_sched(c["p"], c["grads"][0], c["m"], c["v"], lr, B1, B2, EPS, wd, s.current)
    assert not _equal(c["p"], keep["p"])


# ---- the optimizer ------------------------------------------------------------------------------------------------------
def _distinct_ids(batch, cfg, seed=3):
    """No token id more than once: the word table's gradient is a float-atomic scatter-add, whose last bits depend on the order of
    three or more addends -- with distinct ids every gradient of the step is reproducible, so two runs can be compared bit for bit."""
    ids = batch["input_ids"]
    g = torch.Generator().manual_seed(seed)
    perm = 5 + torch.randperm(cfg.vocab_size - 5, generator=g)[:ids.numel()]
    return dict(batch, input_ids=perm.view(ids.shape).to(ids.device, ids.dtype))


def _groups(m):
    from mtvaf_amd.optim import finetune_param_groups
    return finetune_param_groups(m, 1e-3, layer_lr_decay=0.9)  # two groups inside every encoder layer: segmented launches


def _eager_steps(m, opt, sched, batch, steps):
    from mtvaf_amd import engine
    for _ in range(steps):
        with engine.padding_free(False):
            m(**batch).loss.backward()
        opt.step()
        if sched is not None:
            sched.step()
        opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()


def _assert_same_training_state(m1, o1, m2, o2, what):
    for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert _equal(p, q), (what, n)
    s1, s2 = o1.state_dict(), o2.state_dict()
    assert s1["param_groups"] == s2["param_groups"], what
    assert set(s1["state"]) == set(s2["state"]) and len(s1["state"]) > 20
    for k, a in s1["state"].items():
        b = s2["state"][k]
        assert set(a) == set(b), (what, k)
        for name, x in a.items():
            if name in ("step", "ema_step"):
                assert int(x) == int(b[name]), (what, k, name, x, b[name])
            else:
                assert _equal(x, b[name]), (what, k, name)


@pytest.mark.parametrize("extras", [{}, dict(max_grad_norm=0.5, ema_decay=DECAY)], ids=["plain", "clip_ema"])
def test_optimizer_on_the_device_schedule_equals_adamw_with_lambdalr_and_survives_a_checkpoint(extras):
    from mtvaf_amd.optim import AdamW, ScheduleMirror, schedule_table
    factor, T = _factor(), 7
    batch = _distinct_ids(_batch(), TINY["cfg"])
    m1, m2 = _model(), _model()
    o1 = AdamW(_groups(m1), model=m1, **extras)
    s1 = torch.optim.lr_scheduler.LambdaLR(o1, factor)
    table = schedule_table(factor, T, (B1, B2), ema_decay=extras.get("ema_decay", 0.0))
    o2 = AdamW(_groups(m2), model=m2, device_schedule=table, **extras)
    s2 = ScheduleMirror(o2)
    _eager_steps(m1, o1, s1, batch, 5)
    _eager_steps(m2, o2, s2, batch, 5)
    assert o2.schedule_count == 5 == int(o2._sched_dev["counter"])
    o2.assert_schedule_agrees()
    _assert_same_training_state(m1, o1, m2, o2, "5 steps")
    assert not _equal(m1.fc.weight, _model().fc.weight)
    if extras:
        assert float(o1.last_grad_norm) == float(o2.last_grad_norm) > 0
    # a checkpoint into a fresh optimizer on the device schedule, two more steps of both
    sd = copy.deepcopy(o2.state_dict())
    o3 = AdamW(_groups(m2), model=m2, device_schedule=schedule_table(factor, T, (B1, B2), ema_decay=extras.get("ema_decay", 0.0)), **extras)
    o3.load_state_dict(sd)
    assert o3.schedule_count == 5
    s3 = ScheduleMirror(o3)
    o3.assert_schedule_agrees()
    _eager_steps(m1, o1, s1, batch, 2)
    _eager_steps(m2, o3, s3, batch, 2)
    assert o3.schedule_count == 7 == int(o3._sched_dev["counter"])
    _assert_same_training_state(m1, o1, m2, o3, "after the checkpoint")
    # the table is used up: the host mirror raises before anything is launched
    m2(**batch).loss.backward()
    before = m2.fc.weight.detach().clone()
    with pytest.raises(RuntimeError, match="past the end"):
        o3.step()
    torch.cuda.synchronize()
    assert _equal(before, m2.fc.weight) and int(o3._sched_dev["counter"]) == 7


# 128 token rows of hidden 128: whole 128-row tiles, so the bf16 mode runs on bf16 operands and the update writes their shadows
GRAPH_SHAPE = dict(cfg=P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64), B=2, S=64)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_whole_step_graph_with_the_optimizer_inside_equals_the_eager_steps(dtype):
    from mtvaf_amd import engine
    from mtvaf_amd.graph import GraphedTrainStep
    from mtvaf_amd.optim import AdamW, ScheduleMirror, schedule_table
    factor, T = _factor(), 5
    extras = dict(max_grad_norm=0.5, ema_decay=DECAY)
    with _compute(dtype):
        # eval mode and dropout 0, as test_graphed_training_trajectory_equals_eager: the model-level nn.Dropout modules would draw
        # different host-seeded masks in the two models
        m1, m2 = _model(GRAPH_SHAPE), _model(GRAPH_SHAPE)
        batch = _distinct_ids(_batch(GRAPH_SHAPE), GRAPH_SHAPE["cfg"])
        o1 = AdamW(_groups(m1), model=m1, **extras)
        s1 = torch.optim.lr_scheduler.LambdaLR(o1, factor)
        with pytest.raises(RuntimeError, match="device_schedule"):
            GraphedTrainStep(m1, batch, optimizer=o1)
        o2 = AdamW(_groups(m2), model=m2, device_schedule=schedule_table(factor, T, (B1, B2), ema_decay=DECAY), **extras)
        s2 = ScheduleMirror(o2)
        start = {n: p.detach().clone() for n, p in m2.named_parameters()}
        g = GraphedTrainStep(m2, batch, optimizer=o2)
        try:
            torch.cuda.synchronize()
            # the warm-up passes and the capture trained nothing: the first replay is update number 1
            assert o2.schedule_count == 0 == int(o2._sched_dev["counter"]) and int(o2.skipped_steps) == 0
            for n, p in m2.named_parameters():
                assert _equal(p, start[n]), n
            norms = []
            for t in range(1, 6):
                with engine.padding_free(False):
                    m1(**batch).loss.backward()
                o1.step()
                s1.step()
                o1.zero_grad(set_to_none=True)
                out = g(**batch)
                s2.step()
                o2.zero_grad(set_to_none=True)  # legal: the next replay re-attaches the graph's gradient tensors
                norms.append((float(o1.last_grad_norm), float(o2.last_grad_norm)))
                assert o2.schedule_count == t
            torch.cuda.synchronize()
            # (update 1 runs at lr factor 0 -- the warm-up starts there -- so steps 1 and 2 see the same parameters and the same norm)
            assert all(a == b > 0 for a, b in norms) and len({a for a, _ in norms}) == 4, norms
            assert int(o2._sched_dev["counter"]) == 5
            o2.assert_schedule_agrees()
            _assert_same_training_state(m1, o1, m2, o2, "5 replays")
            assert not _equal(m2.fc.weight, start["fc.weight"])
            if dtype == "bf16":
                for store in m2.bert.encoder._stores:  # the captured update wrote the GEMM operand image of the new masters
                    sh = engine.shadow_for_update(store.weights)
                    assert sh is not None and _equal(sh, store.flat.to(torch.bfloat16))
            # past the 5-row table: the host raises and launches nothing
            after = {n: p.detach().clone() for n, p in m2.named_parameters()}
            with pytest.raises(RuntimeError, match="past the end"):
                g(**batch)
            torch.cuda.synchronize()
            assert o2.schedule_count == 5 == int(o2._sched_dev["counter"])
            for n, p in m2.named_parameters():
                assert _equal(p, after[n]), n
            with pytest.raises(RuntimeError, match="captured"):
                o2.step()
        finally:
            g.close()
        assert o2._graphed is None
