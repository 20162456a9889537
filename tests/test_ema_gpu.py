"""The averaged weights (EMA) kept by the AdamW update kernels on the MI355X (the *_ema entry points and mtvaf_swap_f32_multi of
csrc/optim.hip; mtvaf_amd.optim.AdamW(ema_decay=...)): the update itself must not notice the average, the average must follow the
float64 restatement of ema_cases.py within its derived bound, a skipped step must leave it alone, and swapping it in must give the
model that ema_state_dict() describes."""
import contextlib
import copy
import ctypes
import math

import pytest
import torch

import ema_cases as EC
import params as P
from optim_trace import recorded_updates as _recorded_updates
from test_model_gpu import DEV, LABELS, _prompt_inputs, hf_config, make_args

pytestmark = pytest.mark.gpu

CLIPS = {"host": None, "dev": 1.0, "dev_half": 0.5}  # the clip coefficient of the clip_state forms (finite = 1)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.uint8 if t.element_size() == 1 else torch.int32))


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _clip_state(coef, finite=1.0):
    return None if coef is None else torch.tensor([1.0, coef, finite, 0.0], device=DEV)


def _buf(x, offset):
    """x on the device at a 16-byte boundary, or 4 bytes behind one."""
    if not offset:
        t = x.to(DEV).clone()
        assert t.data_ptr() % 16 == 0
        return t
    t = torch.cat([x.new_zeros(1), x]).to(DEV)[1:]
    assert t.data_ptr() % 16 == 4
    return t


def _case(n, seed):
    g = torch.Generator().manual_seed(seed)
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 0.01
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(EC.STEPS)]
    return p, m, v, grads


def _run_flat(n, offsets, max_blocks, coef, with_ema, seed=1):
    """STEPS calls of hip.adamw (bf16 shadow included) -> per step (p, m, v, shadow, e) clones; e is None without the average."""
    from mtvaf_amd import hip
    p0, m0, v0, grads = _case(n, seed)
    p, m, v = _buf(p0, "p" in offsets), _buf(m0, False), _buf(v0, False)
    e = _buf(torch.zeros(n), "e" in offsets) if with_ema else None
    sh = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    clip = _clip_state(coef)
    out = []
    for t, omd in enumerate(EC.step_omds()):
        kw = dict(ema=e, ema_omd=omd) if with_ema else {}
        hip.adamw(p, grads[t].to(DEV), m, v, *EC.HYPER, t + 1, p_bf16=sh, max_blocks=max_blocks, clip=clip, **kw)
        out.append(tuple(None if x is None else x.clone() for x in (p, m, v, sh, e)))
    return out


def _check_average(steps, what):
    """e of every step against the float64 recurrence over the kernel's own p; -> the worst error in units of the bound."""
    ref = EC.Ema64(steps[0][0])
    worst = 0.0
    for t, (omd, snap) in enumerate(zip(EC.step_omds(), steps)):
        p, e = snap[0], snap[-1]
        ref.step(p, EC.as_f32(omd))
        if t == 0:
            assert _same(e, p), (what, "the first update (omd = 1) must make the average the parameter exactly")
        w = ref.worst(e)
        worst = max(worst, w)
        assert w <= 1.0, (what, t, w, ref.worst_last_values(e))
    return worst


# ---- the kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", list(EC.ALIGNMENTS))
def test_flat_update_with_the_average_is_the_update_without_it_and_the_average_follows_float64(align):
    """mtvaf_adamw_ema, host-scalar and clip_state forms, every length / alignment / grid at which the body switches: p, m, v and the
    bf16 shadow are the bits of the call without `ema` after every step, and e stays within the bound."""
    offsets = EC.ALIGNMENTS[align]
    worst = 0.0
    for n in EC.LENGTHS:
        for blocks in EC.MAX_BLOCKS:
            for name, coef in CLIPS.items():
                plain = _run_flat(n, offsets, blocks, coef, False)
                ema = _run_flat(n, offsets, blocks, coef, True)
                for t, (a, b) in enumerate(zip(plain, ema)):
                    for k in range(4):
                        assert _same(a[k], b[k]), (n, blocks, name, t, "pmvs"[k])
                assert not _same(plain[0][0], plain[-1][0]) and not bool((ema[-1][3] == 7.0).all())  # (the calls did update)
                worst = max(worst, _check_average(ema, (n, blocks, name)))
    # the coefficient did reach the update: another trajectory
    assert not _same(_run_flat(1027, offsets, 0, 0.5, False)[-1][1], _run_flat(1027, offsets, 0, 1.0, False)[-1][1])
    print(f"[{align}] worst |e - e64| in units of 2 T 2^-23 max(|p|, |e|): {worst:.3f}")


def _multi_buffers(with_ema, seed=2):
    g = torch.Generator().manual_seed(seed)
    ps, ms, vs, es, grads = [], [], [], [], []
    for i, n in enumerate(EC.MULTI_LENGTHS):
        ps.append(_buf(torch.randn(n, generator=g), i % 7 == 3))   # some parameters and some averages 4 bytes off
        ms.append(_buf(torch.randn(n, generator=g) * 0.01, False))
        vs.append(_buf(torch.rand(n, generator=g) * 0.01, False))
        es.append(_buf(torch.zeros(n), i % 5 == 2) if with_ema else None)
        grads.append([(torch.randn(n, generator=g) * 0.1).to(DEV) for _ in range(EC.STEPS)])
    return ps, ms, vs, es, grads


def _run_multi(coef, with_ema):
    from mtvaf_amd import hip
    ps, ms, vs, es, grads = _multi_buffers(with_ema)
    clip = _clip_state(coef)
    out = []
    for t, omd in enumerate(EC.step_omds()):
        kw = dict(ema=es, ema_omd=omd) if with_ema else {}
        hip.adamw_multi(ps, [g[t] for g in grads], ms, vs, *EC.HYPER, t + 1, clip=clip, **kw)
        out.append([tuple(None if x is None else x.clone() for x in (p, m, v, e)) for p, m, v, e in zip(ps, ms, vs, es)])
    return out


@pytest.mark.parametrize("form", list(CLIPS))
def test_multi_update_of_49_tensors_with_the_average(form):
    """mtvaf_adamw_multi_ema across the 48-tensor launch boundary, lengths from 1 to 65540, some bases 4 bytes off."""
    plain, ema = _run_multi(CLIPS[form], False), _run_multi(CLIPS[form], True)
    worst = 0.0
    for i, n in enumerate(EC.MULTI_LENGTHS):
        for t in range(EC.STEPS):
            for k in range(3):
                assert _same(plain[t][i][k], ema[t][i][k]), (i, n, t, "pmv"[k])
        assert not _same(ema[0][i][0], ema[-1][i][0]), (i, n)  # tensor 49 (the second launch) was updated too
        worst = max(worst, _check_average([s[i] for s in ema], (form, i, n)))
    print(f"[{form}] worst |e - e64| in units of the bound over 49 tensors: {worst:.3f}")


def _run_planes(coef, with_ema, max_blocks=0, finite=1.0, seed=3):
    from mtvaf_amd import hip
    n = EC.PLANE_N
    p0, m0, v0, grads = _case(n, seed)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    e = torch.zeros(n, device=DEV) if with_ema else None
    segs = [(b, r, c, torch.full((6 * r * c,), 0x7f, dtype=torch.uint8, device=DEV)) for b, r, c in EC.PLANE_SEGS]
    clip = _clip_state(coef, finite)
    out = []
    for t, omd in enumerate(EC.step_omds()):
        kw = dict(ema=e, ema_omd=omd) if with_ema else {}
        hip.adamw_planes(p, grads[t].to(DEV), m, v, *EC.HYPER, t + 1, segs, max_blocks=max_blocks, clip=clip, **kw)
        out.append(tuple(x.clone() for x in (p, m, v)) + tuple(s[3].clone() for s in segs) + (None if e is None else e.clone(),))
    return out


@pytest.mark.parametrize("form", list(CLIPS))
def test_planes_update_with_the_average(form):
    """mtvaf_adamw_planes_ema on four of the smallest matrices with stretches outside every matrix: parameters, moments and all four
    plane images are the bits of the call without `ema`; the average covers the stretches too."""
    from mtvaf_amd import hip
    for blocks in EC.MAX_BLOCKS:
        plain, ema = _run_planes(CLIPS[form], False, blocks), _run_planes(CLIPS[form], True, blocks)
        for t, (a, b) in enumerate(zip(plain, ema)):
            for k in range(7):
                assert _same(a[k], b[k]), (blocks, t, k)
        assert all(not bool((img == 0x7f).all()) for img in ema[-1][3:7])
        # the images are those of a split pass over the updated matrices: the average fed nothing into them
        p = ema[-1][0]
        for (b, r, c), img in zip(EC.PLANE_SEGS, ema[-1][3:7]):
            want = torch.empty_like(img)
            hip.split_planes_blocked(p[b:b + r * c].view(r, c).contiguous(), want)
            assert _same(img, want), (b, r, c)
        w = _check_average(ema, (form, blocks))
        print(f"[{form}, max_blocks {blocks}] worst |e - e64| in units of the bound: {w:.3f}")


def test_a_clip_state_that_is_not_finite_leaves_the_average_with_everything_else():
    from mtvaf_amd import hip
    skip = torch.tensor([float("inf"), 0.0, 0.0, 0.0], device=DEV)
    g = torch.Generator().manual_seed(9)
    for n, off in ((1027, False), (1027, True), (4, False)):
        p, m, v, e = (_buf(torch.randn(n, generator=g), off) for _ in range(4))
        sh = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
        gr = torch.randn(n, generator=g).to(DEV)
        keep = [t.clone() for t in (p, m, v, e, sh)]
        hip.adamw(p, gr, m, v, *EC.HYPER, 2, p_bf16=sh, clip=skip, ema=e, ema_omd=0.1)
        hip.adamw_multi([p], [gr], [m], [v], *EC.HYPER, 2, clip=skip, ema=[e], ema_omd=0.1)
        for a, b in zip(keep, (p, m, v, e, sh)):
            assert _same(a, b), n
    frozen = _run_planes(0.0, True, finite=0.0)
    p0, m0, v0, _ = _case(EC.PLANE_N, 3)
    last = frozen[-1]
    assert _same(last[0], p0.to(DEV)) and _same(last[1], m0.to(DEV)) and _same(last[2], v0.to(DEV))
    assert all(bool((img == 0x7f).all()) for img in last[3:7]) and not bool(last[7].any())


def test_ema_entry_points_refuse_bad_arguments_and_write_nothing():
    from mtvaf_amd import hip
    L = hip.lib()
    n = 64
    p, g, m, v, e = (torch.randn(n, device=DEV) for _ in range(5))
    v.abs_()
    keep = [t.clone() for t in (p, m, v, e)]
    ptr = lambda t: t.data_ptr()
    st = hip._st()
    base = (ptr(p), ptr(g), ptr(m), ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.03, 1.0)
    arr = lambda *ts: (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) or t is None else ptr(t) for t in ts])
    ns = (ctypes.c_long * 1)(n)
    img = torch.zeros(6 * 64, dtype=torch.uint8, device=DEV)
    seg = ((ctypes.c_long * 1)(0), (ctypes.c_int * 1)(2), (ctypes.c_int * 1)(32), arr(img))
    for ema_ptr, omd in ((None, 0.1), (ptr(e), -0.01), (ptr(e), 1.5), (ptr(e), float("nan"))):
        assert L.mtvaf_adamw_ema(*base, None, 0, ema_ptr, omd, None, st) == -3
        assert L.mtvaf_adamw_planes_ema(*base, 1, *seg, 0, ema_ptr, omd, None, st) == -3
        assert L.mtvaf_adamw_multi_ema(1, arr(p), arr(g), arr(m), arr(v), ns, *base[5:], arr(ema_ptr) if ema_ptr else None, omd, None,
                                       st) == -3
    assert L.mtvaf_adamw_multi_ema(1, arr(p), arr(g), arr(m), arr(v), ns, *base[5:], arr(None), 0.1, None, st) == -3
    assert L.mtvaf_adamw_ema(*base, None, 0, ptr(e) + 2, 0.1, None, st) == -2  # not a float boundary
    assert L.mtvaf_adamw_planes_ema(*base, 1, *seg, 0, ptr(e) + 4, 0.1, None, st) == -2  # the planes form wants 16 bytes
    torch.cuda.synchronize()
    for a, b in zip(keep, (p, m, v, e)):
        assert _same(a, b)
    # the ends of the interval are legal: 0 leaves the average alone, 1 makes a zero average the new parameter exactly
    e.zero_()
    assert L.mtvaf_adamw_ema(*base, None, 0, ptr(e), 0.0, None, st) == 0 and L.mtvaf_adamw_ema(*base, None, 0, ptr(e), 1.0, None, st) == 0
    torch.cuda.synchronize()
    assert _same(e, p)


# ---- the exchange -------------------------------------------------------------------------------------------------------
def test_swap_exchanges_bit_for_bit_and_twice_is_the_identity():
    from mtvaf_amd import hip
    g = torch.Generator().manual_seed(4)
    a, b = [], []
    for i, n in enumerate(EC.MULTI_LENGTHS):  # 49 pairs: two launches; every switching length; either side 4 bytes off for some
        a.append(_buf(torch.randn(n, generator=g), i % 7 == 3 or i < 6 and i % 2 == 1))
        b.append(_buf(torch.randn(n, generator=g), i % 5 == 2))
    a[0].view(torch.int32).fill_(0x7fc12345)  # a NaN with a payload travels as bits
    a0, b0 = [t.clone() for t in a], [t.clone() for t in b]
    hip.swap_f32(a, b)
    for i in range(len(a)):
        assert _same(a[i], b0[i]) and _same(b[i], a0[i]), (i, EC.MULTI_LENGTHS[i])
    hip.swap_f32(a, b)
    for i in range(len(a)):
        assert _same(a[i], a0[i]) and _same(b[i], b0[i]), (i, EC.MULTI_LENGTHS[i])
    for n in EC.LENGTHS:  # one pair at a time, both sides aligned: the float4 body and its tail
        x, y = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
        x0, y0 = x.clone(), y.clone()
        hip.swap_f32([x], [y])
        assert _same(x, y0) and _same(y, x0), n


def test_swap_refuses_overlapping_and_null_arguments_and_writes_nothing():
    from mtvaf_amd import hip
    L = hip.lib()
    buf = torch.randn(64, device=DEV)
    other = torch.randn(32, device=DEV)
    keep = (buf.clone(), other.clone())
    one = lambda x: (ctypes.c_void_p * 1)(x)
    n32, st = (ctypes.c_long * 1)(32), hip._st()
    base = buf.data_ptr()
    assert L.mtvaf_swap_f32_multi(1, one(base), one(base + 4 * 16), n32, st) == -3      # b starts inside a
    assert L.mtvaf_swap_f32_multi(1, one(base + 4 * 31), one(base), n32, st) == -3      # a starts in b's last element
    assert L.mtvaf_swap_f32_multi(1, one(base), one(base), n32, st) == -3               # the same buffer
    assert L.mtvaf_swap_f32_multi(1, one(None), one(base), n32, st) == -3
    assert L.mtvaf_swap_f32_multi(1, one(base), one(None), n32, st) == -3
    assert L.mtvaf_swap_f32_multi(1, None, one(base), n32, st) == -3
    assert L.mtvaf_swap_f32_multi(1, one(base), one(other.data_ptr()), None, st) == -3
    assert L.mtvaf_swap_f32_multi(1, one(base), one(other.data_ptr()), (ctypes.c_long * 1)(0), st) == -3
    assert L.mtvaf_swap_f32_multi(-1, one(base), one(other.data_ptr()), n32, st) == -3
    # a good pair in front of a bad one: the whole call is refused before the first launch
    two = lambda x, y: (ctypes.c_void_p * 2)(x, y)
    assert L.mtvaf_swap_f32_multi(2, two(base, base + 4 * 40), two(other.data_ptr(), base + 4 * 44), (ctypes.c_long * 2)(32, 8), st) == -3
    torch.cuda.synchronize()
    assert _same(buf, keep[0]) and _same(other, keep[1])
    assert L.mtvaf_swap_f32_multi(0, None, None, None, st) == 0
    assert L.mtvaf_swap_f32_multi(1, one(base), one(base + 4 * 32), n32, st) == 0       # adjacent halves do not overlap
    torch.cuda.synchronize()
    assert _same(buf[:32], keep[0][32:]) and _same(buf[32:], keep[0][:32])


# ---- the optimizer ------------------------------------------------------------------------------------------------------
DECAY = 0.9
MODES = ["planes", "flat", "bf16"]  # fp32 pre-split operands (the planes form), fp32 without them (the flat form), bf16 (the shadow form)
# one encoder matrix, one LayerNorm vector, the word table, the heads (and every other trained parameter is checked with them)
MUST_CHECK = ["bert.encoder.layer.1.intermediate.dense.weight", "bert.encoder.layer.0.attention.output.LayerNorm.weight",
              "bert.embeddings.word_embeddings.weight", "fc.weight", "crf.transitions"]


@contextlib.contextmanager
def _mode(mode):
    from mtvaf_amd import engine, hip
    was_c, was_p = hip.COMPUTE, engine.F32_PLANES
    hip.set_compute_dtype("bf16" if mode == "bf16" else "fp32")
    engine.F32_PLANES = was_p and mode != "flat"
    try:
        yield
    finally:
        engine.F32_PLANES = was_p
        hip.set_compute_dtype(was_c)


def _model():
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
    args = make_args(alpha=0.0)
    args.bert_config = hf_config(cfg, dropout=0.0)
    torch.manual_seed(11)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    m.eval()
    return m, cfg


def _batch(cfg, B=16, S=64, seed=5):
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, seed, B, S, lo_id=5))
    feats, aux, _ = (t.to(DEV) for t in _prompt_inputs(seed + 1, B, 3))
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats, aux_imgs=aux)


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _emas(m, opt):
    return {n: opt.state[p]["ema"].detach().clone() for n, p in m.named_parameters() if p in opt.state and "ema" in opt.state[p]}


def _one_step(m, opt, batch):
    m(**batch).loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)


def _train(steps=3, m=None, opt=None, first=0, **kw):
    """-> model, optimizer, per-step parameter and average snapshots of `steps` steps on the fixed batch."""
    from mtvaf_amd.optim import AdamW
    if m is None:
        m, cfg = _model()
        opt = AdamW(m.parameters(), lr=1e-3, model=m, **kw)
    batch = _batch(P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64))
    ps, es = [], []
    for _ in range(first, steps):
        _one_step(m, opt, batch)
        ps.append(_params(m))
        es.append(_emas(m, opt))
    torch.cuda.synchronize()
    return m, opt, ps, es


def _check_trajectory(ps, es, decay=DECAY, warmup=True):
    """The averages of every step against the float64 recurrence over the recorded parameters; -> the worst error in units of the
    bound, and the names checked."""
    names = sorted(es[-1])
    assert set(MUST_CHECK) <= set(names), sorted(set(MUST_CHECK) - set(names))
    ref = {n: EC.Ema64(ps[0][n]) for n in names}
    worst, last = 0.0, 0.0
    for t in range(len(ps)):
        omd = EC.omd32(EC.decay_at(t, decay, warmup))
        for n in names:
            ref[n].step(ps[t][n], omd)
            if t == 0:
                assert _same(es[0][n], ps[0][n]), n  # the average starts as the parameters after their first update, exactly
            w = ref[n].worst(es[t][n])
            last = max(last, ref[n].worst_last_values(es[t][n]))
            assert w <= 1.0, (n, t, w)
            worst = max(worst, w)
    print(f"(in units of the last step's magnitudes alone: {last:.3f})")
    return worst, names


@pytest.fixture(scope="module")
def plain_runs():
    """Three steps without the average, per mode: shared, read-only."""
    out = {}
    for mode in MODES:
        with _mode(mode):
            out[mode] = _train(ema_decay=0.0)[2]
    return out


@pytest.fixture(scope="module")
def ema_runs():
    """Three steps with ema_decay = 0.9, overlap = False, per mode -> (parameter snapshots, average snapshots, update calls)."""
    out = {}
    for mode in MODES:
        with _mode(mode), _recorded_updates() as calls:
            _, opt, ps, es = _train(ema_decay=DECAY)
            out[mode] = (ps, es, list(calls), None)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_optimizer_with_the_average_trains_the_same_bits_and_the_average_follows_float64(mode, plain_runs, ema_runs):
    ps, es, calls, _ = ema_runs[mode]
    layer_calls = [c for c in calls if c[0] in ("adamw", "adamw_planes")]
    assert len(layer_calls) == 2 * 3 and all(c[1] for c in calls) and any(c[0] == "adamw_multi" for c in calls)
    want = {"planes": ("adamw_planes", False), "flat": ("adamw", False), "bf16": ("adamw", True)}[mode]
    assert all((c[0], c[2]) == want for c in layer_calls), layer_calls  # the form of the update this mode is about
    for t in range(3):
        for n, p in plain_runs[mode][t].items():
            assert _same(ps[t][n], p), (t, n)
    assert not _same(ps[0]["fc.weight"], ps[2]["fc.weight"])
    worst, names = _check_trajectory(ps, es)
    print(f"[{mode}] {len(names)} averaged tensors, worst |e - e64| in units of the bound: {worst:.3f}")


@pytest.mark.parametrize("mode", ["planes", "bf16"])
def test_overlap_inside_backward_gives_the_bits_of_the_plain_schedule(mode, ema_runs):
    with _mode(mode), _recorded_updates() as calls:
        m, opt, ps, es = _train(ema_decay=DECAY, overlap=True)
    assert opt.overlap and m.bert.encoder.grad_sink.on_layer_done is not None and all(c[1] for c in calls)
    rp, re_, _, _ = ema_runs[mode]
    for t in range(3):
        for n in rp[t]:
            assert _same(ps[t][n], rp[t][n]), (t, n)
        assert es[t].keys() == re_[t].keys()
        for n in re_[t]:
            assert _same(es[t][n], re_[t][n]), (t, n)


def test_with_a_bound_the_average_follows_the_clipped_trajectory_and_a_skipped_step_leaves_it(plain_runs):
    m0, _ = _model()
    batch = _batch(P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64))
    m0(**batch).loss.backward()
    n0 = float(torch.nn.utils.clip_grad_norm_(m0.parameters(), 1e30))
    with _recorded_updates() as calls:
        m, opt, ps, es = _train(ema_decay=DECAY, max_grad_norm=0.5 * n0)
    assert calls and all(c[1] and c[3] for c in calls)  # every update: with the average, under the device clip state
    assert int(opt.skipped_steps) == 0
    assert not _same(ps[2]["bert.encoder.layer.1.intermediate.dense.weight"],
                     plain_runs["planes"][2]["bert.encoder.layer.1.intermediate.dense.weight"])  # the bound did clip
    worst, _ = _check_trajectory(ps, es)
    print(f"clipped run: worst |e - e64| in units of the bound: {worst:.3f}")
    # a non-finite gradient: the step is dropped, the averages keep their bits, the skip is counted; the host counter moves on
    w = m.bert.encoder.layer[1].intermediate.dense.weight
    count = int(opt.state[w]["ema_step"])
    assert count == 3 == int(opt.state[m.fc.weight]["ema_step"])
    m(**batch).loss.backward()
    w.grad[3, 5] = float("inf")
    opt.step()
    opt.zero_grad(set_to_none=True)
    after_p, after_e = _params(m), _emas(m, opt)
    assert int(opt.skipped_steps) == 1 and not math.isfinite(float(opt.last_grad_norm))
    for n in es[2]:
        assert _same(after_e[n], es[2][n]) and _same(after_p[n], ps[2][n]), n
    assert int(opt.state[w]["ema_step"]) == count + 1  # (the documented caveat, as for the bias correction)
    _one_step(m, opt, batch)
    assert int(opt.skipped_steps) == 1 and not _same(_emas(m, opt)["fc.weight"], es[2]["fc.weight"])


def _forward(m, batch):
    with torch.no_grad():
        out = m(**batch)
    return out.loss.detach().clone(), out.logits


@pytest.mark.parametrize("mode", ["planes", "bf16"])
def test_swap_ema_gives_the_model_of_ema_state_dict_and_swapping_back_continues_the_run(mode, ema_runs):
    rp, re_, _, _ = ema_runs[mode]
    with _mode(mode):
        m, opt, ps, es = _train(steps=2, ema_decay=DECAY)
        batch = _batch(P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64))
        sd = opt.ema_state_dict(m)
        for n in MUST_CHECK:
            assert _same(sd[n], es[1][n]) and not _same(sd[n], ps[1][n]), n
        frozen = [n for n, p in m.named_parameters() if n not in es[1]]
        assert all(_same(sd[n], ps[1][n]) for n in frozen)  # no average: the parameter's own value
        assert sd.keys() == m.state_dict().keys()
        train_loss, _ = _forward(m, batch)
        opt.swap_ema()
        assert opt.ema_swapped
        for n in MUST_CHECK:  # the parameters hold the averages, the state holds the training weights
            assert _same(dict(m.named_parameters())[n], es[1][n]) and _same(_emas(m, opt)[n], ps[1][n]), n
        assert all(_same(v, sd[k]) for k, v in opt.ema_state_dict(m).items())  # swapped in: the parameters ARE the averages
        loss_a, tags_a = _forward(m, batch)
        fresh, _ = _model()
        fresh.load_state_dict(sd)
        loss_b, tags_b = _forward(fresh, batch)
        print(f"[{mode}] loss on the averaged weights {float(loss_a)!r}, fresh model {float(loss_b)!r}, training weights {float(train_loss)!r}")
        assert _same(loss_a, loss_b) and tags_a == tags_b
        assert not _same(loss_a, train_loss)  # (stale weight images would have reproduced the training weights' loss)
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
        opt.swap_ema()
        assert not opt.ema_swapped
        for n in ps[1]:
            assert _same(dict(m.named_parameters())[n], ps[1][n]), n
        for n in es[1]:
            assert _same(_emas(m, opt)[n], es[1][n]), n
        # an exception inside the block: the training weights are back
        with pytest.raises(KeyError):
            with opt.averaged_parameters():
                assert opt.ema_swapped and _same(m.fc.weight, es[1]["fc.weight"])
                raise KeyError("inside")
        assert not opt.ema_swapped and all(_same(dict(m.named_parameters())[n], ps[1][n]) for n in ps[1])
        loss_c, _ = _forward(m, batch)
        assert _same(loss_c, train_loss)
        # ... and the run goes on as if it had never swapped
        _, _, ps3, es3 = _train(steps=3, m=m, opt=opt, first=2)
    for n in rp[2]:
        assert _same(ps3[0][n], rp[2][n]), n
    for n in re_[2]:
        assert _same(es3[0][n], re_[2][n]), n


def test_overlap_backward_hook_raises_while_swapped():
    m, opt, _, _ = _train(steps=1, ema_decay=DECAY, overlap=True)
    batch = _batch(P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64))
    before = _params(m)
    opt.swap_ema()
    with pytest.raises(RuntimeError, match="swapped in"):
        m(**batch).loss.backward()
    m.zero_grad(set_to_none=True)
    opt.swap_ema()
    torch.cuda.synchronize()
    assert all(_same(p, before[n]) for n, p in m.named_parameters())


def test_checkpoint_round_trip_resumes_parameters_and_averages(ema_runs):
    from mtvaf_amd.optim import AdamW
    rp, re_, _, _ = ema_runs["planes"]
    m, opt, ps, es = _train(steps=2, ema_decay=DECAY)
    sd_o, sd_m = copy.deepcopy(opt.state_dict()), copy.deepcopy(m.state_dict())
    w = "bert.encoder.layer.1.intermediate.dense.weight"
    assert any("ema" in s and "ema_step" in s for s in sd_o["state"].values())
    m2, _ = _model()
    m2.load_state_dict(sd_m)
    opt2 = AdamW(m2.parameters(), lr=1e-3, model=m2, ema_decay=DECAY)
    opt2.load_state_dict(sd_o)
    _, _, ps3, es3 = _train(steps=3, m=m2, opt=opt2, first=2)
    assert int(opt2.state[dict(m2.named_parameters())[w]]["ema_step"]) == 3 == int(opt2.state[m2.fc.weight]["ema_step"])
    for n in rp[2]:
        assert _same(ps3[0][n], rp[2][n]), n
    assert es3[0].keys() == re_[2].keys()
    for n in re_[2]:
        assert _same(es3[0][n], re_[2][n]), n
    # a checkpoint written WITHOUT averages, loaded into an optimizer that keeps them: they start at the next step
    m3, opt3, _, _ = _train(steps=2, ema_decay=0.0)
    m4, _ = _model()
    m4.load_state_dict(copy.deepcopy(m3.state_dict()))
    opt4 = AdamW(m4.parameters(), lr=1e-3, model=m4, ema_decay=DECAY)
    opt4.load_state_dict(copy.deepcopy(opt3.state_dict()))
    _, _, ps4, es4 = _train(steps=3, m=m4, opt=opt4, first=2)
    for n in (w, "fc.weight", "bert.embeddings.word_embeddings.weight"):
        p = dict(m4.named_parameters())[n]
        assert int(opt4.state[p]["step"]) == 3 and int(opt4.state[p]["ema_step"]) == 1
        assert _same(es4[0][n], ps4[0][n]) and _same(ps4[0][n], rp[2][n]), n


def test_defaults_allocate_no_average_and_call_none_of_the_new_entry_points(plain_runs):
    """ema_decay = 0: the wrappers are called exactly as before (no `ema` keyword at all, so they take the branches they always took),
    no state entry, and swap_ema has nothing to swap."""
    from mtvaf_amd import hip
    from mtvaf_amd.optim import AdamW, build_optimizer
    import types
    L = hip.lib()
    new = ("mtvaf_adamw_ema", "mtvaf_adamw_planes_ema", "mtvaf_adamw_multi_ema", "mtvaf_swap_f32_multi")
    hit = []

    class Spy:
        def __getattr__(self, name):
            if name in new:
                hit.append(name)
            return getattr(L, name)
    real_lib = hip.lib
    try:
        hip.lib = lambda: Spy()
        with _recorded_updates() as calls:
            m, opt, ps, es = _train(steps=2)
        assert calls and not any(c[4] for c in calls) and not hit
        assert all("ema" not in s and "ema_step" not in s for s in opt.state.values())
        assert all("ema" not in st for st in opt._flat_state.values()) and opt.ema_decay == 0.0
        for n, p in plain_runs["planes"][1].items():
            assert _same(ps[1][n], p), n
        _train(steps=1, ema_decay=DECAY)
        assert set(hit) == {"mtvaf_adamw_planes_ema", "mtvaf_adamw_multi_ema"}  # (the spy does see the new entry points when they run)
    finally:
        hip.lib = real_lib
    m2, _ = _model()
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, ema_decay=0.99, ema_warmup=False)
    opt2, _ = build_optimizer(m2, args, 100)
    assert isinstance(opt2, AdamW) and opt2.ema_decay == 0.99 and opt2.ema_warmup is False and opt2.overlap is True
    opt3, _ = build_optimizer(_model()[0], types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True), 100)
    assert opt3.ema_decay == 0.0 and opt3.ema_warmup is True
