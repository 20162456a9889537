"""The segmented AdamW update on the MI355X: mtvaf_adamw_seg / mtvaf_adamw_planes_seg (csrc/optim.hip) against the unsegmented
kernels run slice by slice (bit for bit) and against a float64 restatement, and mtvaf_amd.optim.AdamW on parameter groups that
differ inside an encoder layer (finetune_param_groups) against torch.optim.AdamW."""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch

import params as P
from test_model_gpu import DEV, LABELS, _prompt_inputs, hf_config, make_args

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
# 5 segments of a 4099-element buffer (5 blocks of float4s): one 4 elements long, the last one ends at n, and n % 4 == 3 -- the
# scalar tail lies in the last segment
N = 4099
SEGS = [(1024, 1e-3, 1e-2), (1028, 5e-4, 0.0), (2052, 2e-3, 3e-2), (3000, 1e-3, 0.0), (N, 7e-4, 1e-2)]
STEPS = 5


def _same(a, b):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _case(n, seed=1, steps=STEPS):
    g = torch.Generator().manual_seed(seed)
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 0.01
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(steps)]
    return p, m, v, grads


def _run_seg(segs=SEGS, n=N, steps=3, seed=1, **kw):
    """`steps` calls of hip.adamw_seg -> per step (p, m, v) clones."""
    from mtvaf_amd import hip
    p0, m0, v0, grads = _case(n, seed)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    out = []
    for t in range(steps):
        hip.adamw_seg(p, grads[t].to(DEV), m, v, segs, B1, B2, EPS, t + 1, **kw)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


@pytest.fixture(scope="module")
def seg_run():
    """Five steps of the plain segmented update on the 5-segment buffer: shared, read-only."""
    return _run_seg(steps=STEPS)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def test_segmented_update_has_the_bits_of_the_update_run_slice_by_slice(seg_run):
    """The only difference between the two is where lr and weight decay come from: p, m, v equal hip.adamw on each 16-byte
    aligned slice with that segment's (lr, wd), at steps 1 and 3."""
    from mtvaf_amd import hip
    p0, m0, v0, grads = _case(N)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    assert p.data_ptr() % 16 == 0
    for t in range(3):
        g = grads[t].to(DEV)
        lo = 0
        for end, lr, wd in SEGS:
            assert lo % 4 == 0
            hip.adamw(p[lo:end], g[lo:end], m[lo:end], v[lo:end], lr, B1, B2, EPS, wd, t + 1)
            lo = end
        if t in (0, 2):
            for k, (a, b) in enumerate(zip(seg_run[t], (p, m, v))):
                bad = (a != b).nonzero().flatten()
                assert _same(a, b), (t + 1, "pmv"[k], bad[:8].tolist(), int(bad.numel()))
    assert not _same(seg_run[0][0], seg_run[2][0])


def test_uniform_table_has_the_bits_of_the_unsegmented_update():
    from mtvaf_amd import hip
    uniform = [(end, 1e-3, 1e-2) for end, _, _ in SEGS]
    got = _run_seg(uniform)
    p0, m0, v0, grads = _case(N)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    for t in range(3):
        hip.adamw(p, grads[t].to(DEV), m, v, 1e-3, B1, B2, EPS, 1e-2, t + 1)
        for k, (a, b) in enumerate(zip(got[t], (p, m, v))):
            assert _same(a, b), (t + 1, "pmv"[k])
    one = _run_seg([(N, 1e-3, 1e-2)])  # a single segment is the same launch again
    assert all(_same(a, b) for a, b in zip(one[2], got[2]))


def test_segmented_update_follows_float64_adamw_per_segment(seg_run):
    """1 and 5 steps against a float64 restatement of torch.optim.AdamW with each segment's lr and weight decay, at the tolerance
    test_optim_gpu.py uses against torch on parameters (moments: the one it uses on exp_avg)."""
    p0, m0, v0, grads = _case(N)
    p, m, v = p0.double(), m0.double(), v0.double()
    lr = torch.empty(N, dtype=torch.float64)
    wd = torch.empty(N, dtype=torch.float64)
    lo = 0
    for end, l, w in SEGS:
        lr[lo:end], wd[lo:end] = l, w
        lo = end
    for t in range(1, STEPS + 1):
        g = grads[t - 1].double()
        p = p - lr * wd * p
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        p = p - (lr / (1 - B1 ** t)) * m / (v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS)
        if t in (1, STEPS):
            gp, gm, gv = (x.cpu().double() for x in seg_run[t - 1])
            print(f"step {t}: max |p - p64| {float((gp - p).abs().max()):.3e}, |m - m64| {float((gm - m).abs().max()):.3e}, "
                  f"|v - v64| {float((gv - v).abs().max()):.3e}")
            torch.testing.assert_close(gp, p, rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(gm, m, rtol=1e-5, atol=1e-8)
            torch.testing.assert_close(gv, v, rtol=1e-5, atol=1e-8)


def _clip(coef, finite=1.0):
    return torch.tensor([1.0, coef, finite, 0.0], device=DEV)


def test_clip_state_scales_the_gradient_and_a_non_finite_norm_writes_nothing(seg_run):
    from mtvaf_amd import hip
    half = _run_seg(clip=_clip(0.5))
    scaled = _run_seg(grad_scale=0.5)
    for t in range(3):
        assert all(_same(a, b) for a, b in zip(half[t], scaled[t])), t
    assert not _same(half[0][1], seg_run[0][1])  # (the coefficient did reach the update)
    assert all(_same(a, b) for a, b in zip(_run_seg(clip=_clip(1.0))[2], seg_run[2]))
    # finite == 0: parameters, moments, the average and the shadow keep their bits
    p0, m0, v0, grads = _case(N)
    p, m, v, e = p0.to(DEV), m0.to(DEV), v0.to(DEV), torch.randn(N, device=DEV)
    sh = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV)
    keep = [x.clone() for x in (p, m, v, e, sh)]
    hip.adamw_seg(p, grads[0].to(DEV), m, v, SEGS, B1, B2, EPS, 1, p_bf16=sh, clip=_clip(0.0, 0.0), ema=e, ema_omd=0.1)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(keep, (p, m, v, e, sh)))


def test_average_and_shadow_ride_along_without_touching_the_update(seg_run):
    from mtvaf_amd import hip
    p0, m0, v0, grads = _case(N)
    omd = 0.1
    for clip in (None, _clip(1.0)):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        e = torch.randn(N, generator=torch.Generator().manual_seed(7)).to(DEV)
        sh = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV)
        for t in range(3):
            e_old = e.clone()
            hip.adamw_seg(p, grads[t].to(DEV), m, v, SEGS, B1, B2, EPS, t + 1, p_bf16=sh, clip=clip, ema=e, ema_omd=omd)
            for k, (a, b) in enumerate(zip(seg_run[t], (p, m, v))):
                assert _same(a, b), (t + 1, "pmv"[k])
            # e = fmaf(omd, p_new - e, e): the difference rounds to fp32, product and sum round once (exact in double before)
            d = (p - e_old).double()
            want = (float(np.float32(omd)) * d + e_old.double()).float()
            assert _same(e, want), (t + 1, int((e != want).sum()))
            assert _same(sh, p.to(torch.bfloat16)), t + 1


def test_background_grid_has_the_bits_of_the_full_width_launch(seg_run):
    """max_blocks=128 on a buffer that needs 131 blocks (lanes loop), max_blocks=3 on the small one: element-wise arithmetic."""
    n = 4 * 256 * 130 + 7
    segs = [(4 * 256 * 40, 1e-3, 1e-2), (4 * 256 * 40 + 4, 2e-3, 0.0), (n, 5e-4, 1e-2)]
    full, capped = _run_seg(segs, n, steps=2, seed=4), _run_seg(segs, n, steps=2, seed=4, max_blocks=128)
    assert all(_same(a, b) for a, b in zip(full[1], capped[1]))
    assert all(_same(a, b) for a, b in zip(_run_seg(max_blocks=3)[2], seg_run[2]))


# the flat buffer of the plane-image form: two small matrices and two vectors; the third segment ends INSIDE the second matrix
MATS = [(0, 64, 64), (64 * 64 + 64, 64, 128)]
PLANE_N = 64 * 64 + 64 + 64 * 128 + 128
PLANE_SEGS = [(4096, 1e-3, 1e-2), (4160, 1e-3, 0.0), (4160 + 4096, 2e-3, 1e-2), (4160 + 8192, 5e-4, 3e-2), (PLANE_N, 2e-3, 0.0)]


def _run_planes(steps=3, **kw):
    from mtvaf_amd import hip
    p0, m0, v0, grads = _case(PLANE_N, seed=3)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    mats = [(b, r, c, torch.full((6 * r * c,), 0x7f, dtype=torch.uint8, device=DEV)) for b, r, c in MATS]
    for t in range(steps):
        hip.adamw_planes_seg(p, grads[t].to(DEV), m, v, PLANE_SEGS, B1, B2, EPS, t + 1, mats, **kw)
    torch.cuda.synchronize()
    return p, m, v, [x[3] for x in mats]


def test_plane_image_form_has_the_bits_of_the_flat_form_and_the_images_of_the_new_matrices():
    from mtvaf_amd import hip
    flat = _run_seg(PLANE_SEGS, PLANE_N, steps=3, seed=3)[2]
    p, m, v, imgs = _run_planes()
    assert _same(p, flat[0]) and _same(m, flat[1]) and _same(v, flat[2])
    for (b, r, c), img in zip(MATS, imgs):
        want = torch.empty_like(img)
        hip.split_planes_blocked(p[b:b + r * c].view(r, c), want)
        assert torch.equal(img, want), (b, r, c)
    # the options: the average leaves p, m, v and the images alone; a capped grid too; finite == 0 writes nothing
    e = torch.zeros(PLANE_N, device=DEV)
    pe, me, ve, imgs_e = _run_planes(ema=e, ema_omd=1.0, clip=_clip(1.0), max_blocks=3)
    assert _same(pe, p) and _same(me, m) and _same(ve, v) and all(_same(a, b) for a, b in zip(imgs_e, imgs))
    assert _same(e, p)  # (omd = 1: the average is the new parameter exactly)
    p0, m0, v0, _ = _case(PLANE_N, seed=3)
    e.fill_(3.0)
    pz, mz, vz, imgs_z = _run_planes(steps=1, ema=e, ema_omd=0.5, clip=_clip(0.0, 0.0))
    assert _same(pz, p0.to(DEV)) and _same(mz, m0.to(DEV)) and _same(vz, v0.to(DEV)) and bool((e == 3.0).all())
    assert all(bool((img == 0x7f).all()) for img in imgs_z)


def test_bad_segment_tables_are_refused_and_nothing_is_launched():
    from mtvaf_amd import hip
    L = hip.lib()
    n = 64
    p, g, m, v = (torch.randn(n + 16, device=DEV) for _ in range(4))  # (longer than any length a refused call names)
    v.abs_()
    img = torch.full((6 * 2 * 32,), 0x7f, dtype=torch.uint8, device=DEV)
    keep = [t.clone() for t in (p, m, v, img)]
    st = hip._st()
    mat = (1, (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(2), (ctypes.c_int * 1)(32), (ctypes.c_void_p * 1)(img.data_ptr()))

    def call(ends, which, n_=n, k=None):
        k = len(ends) if k is None else k
        head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n_, k, (ctypes.c_long * len(ends))(*ends),
                (ctypes.c_float * len(ends))(*[1e-3] * len(ends)), (ctypes.c_float * len(ends))(*[1e-2] * len(ends)),
                B1, B2, EPS, 0.1, 0.03, 1.0)
        if which == "flat":
            return L.mtvaf_adamw_seg(*head, None, 0, None, 0.0, None, st)
        return L.mtvaf_adamw_planes_seg(*head, *mat, 0, None, 0.0, None, st)

    for which in ("flat", "planes"):
        assert call([4 * (i + 1) for i in range(16)] + [n + 4], which, n_=n + 4) == -3  # 17 segments
        assert call([n], which, k=0) == -3                                              # fewer than 1
        assert call([32, 16, n], which) == -3                                           # decreasing ends
        assert call([16, 16, n], which) == -3                                           # ... or not strictly increasing
        assert call([16, 32], which) == -3                                              # the last end is not n
        assert call([16, n + 4], which) == -3
        assert call([6, n], which) == -3                                                # an inner end of 6
    # an average with 1 - decay outside [0, 1], and bases the float4 body cannot take
    head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1, (ctypes.c_long * 1)(n), (ctypes.c_float * 1)(1e-3),
            (ctypes.c_float * 1)(1e-2), B1, B2, EPS, 0.1, 0.03, 1.0)
    assert L.mtvaf_adamw_seg(*head, None, 0, m.data_ptr(), 1.5, None, st) == -3
    assert L.mtvaf_adamw_seg(*((p.data_ptr() + 4,) + head[1:4] + (n - 4,) + head[5:6] + ((ctypes.c_long * 1)(n - 4),) + head[7:]),
                             None, 0, None, 0.0, None, st) == -2
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(keep, (p, m, v, img)))
    assert call([16, n], "flat") == 0 and call([n], "planes") == 0  # (and good tables are taken)
    torch.cuda.synchronize()
    assert not _same(keep[0], p) and not bool((img == 0x7f).all())


# ---- the optimizer ------------------------------------------------------------------------------------------------------
TINY = dict(cfg=P.EncCfg(vocab_size=600, hidden=64, heads=1, inter=128, layers=2, max_pos=64), B=2, S=8)
# 1024 token rows of hidden 128: where a forward pass builds the weights' plane images (fp32) or their bf16 shadows
WIDE = dict(cfg=P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64), B=16, S=64)
SEG_CALLS = ("adamw_seg", "adamw_planes_seg")


def _model(shape=TINY):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(alpha=0.0)
    args.bert_config = hf_config(shape["cfg"], dropout=0.0)
    torch.manual_seed(11)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    m.eval()
    return m


def _batch(shape=TINY, seed=5):
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(shape["cfg"], seed, shape["B"], shape["S"], lo_id=5))
    feats, aux, _ = (t.to(DEV) for t in _prompt_inputs(seed + 1, shape["B"], 3))
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats, aux_imgs=aux)


@contextlib.contextmanager
def _recorded():
    """The update wrappers the optimizer calls, recorded as (name, args, kwargs)."""
    from mtvaf_amd import hip
    calls = []
    real = {k: getattr(hip, k) for k in ("adamw", "adamw_planes", "adamw_multi") + SEG_CALLS}

    def wrap(name):
        def f(*a, **k):
            calls.append((name, a, k))
            return real[name](*a, **k)
        return f
    try:
        for k in real:
            setattr(hip, k, wrap(k))
        yield calls
    finally:
        for k, f in real.items():
            setattr(hip, k, f)


def _steps(m, opt, batch, steps=3, sched=None, after_backward=None):
    losses = []
    for _ in range(steps):
        out = m(**batch)
        out.loss.backward()
        if after_backward is not None:
            after_backward()
        opt.step()
        if sched is not None:
            sched.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(out.loss.detach()))
    torch.cuda.synchronize()
    return losses


def _assert_params_close(m, ref, skip=("key.bias", "word_embeddings")):
    """The bounds of test_build_optimizer_with_gradient_accumulation_equals_torch_adamw (and what it leaves out: a pure-noise
    gradient whose sign Adam amplifies, a float-atomic scatter-add)."""
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if any(s in n for s in skip):
            continue
        atol = 2.5e-4 if (n.startswith("crf") or n.startswith("fc")) else 5e-6
        torch.testing.assert_close(p, q, rtol=0, atol=atol, msg=lambda s, n=n: f"{n}: {s}")


def _layer_ptrs(m):
    return {p.data_ptr() for layer in m.bert.encoder.layer for p in layer.ordered_params()}


@pytest.mark.parametrize("shape", ["tiny", "wide"])
def test_hf_style_groups_take_one_segmented_launch_per_layer_and_equal_torch_adamw(shape):
    """finetune_param_groups (biases / LayerNorm weights without weight decay, lr decaying with depth): after 3 steps every parameter
    equals torch.optim.AdamW on the same groups; every encoder layer takes exactly ONE segmented launch per step and none of its
    tensors reaches adamw_multi.  `wide` is where the layers' plane images are live, so the launch is the plane-image form."""
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    shape = {"tiny": TINY, "wide": WIDE}[shape]
    m = _model(shape)
    ref = copy.deepcopy(m)
    ours = AdamW(finetune_param_groups(m, 1e-3, layer_lr_decay=0.9), model=m)
    topt = torch.optim.AdamW(finetune_param_groups(ref, 1e-3, layer_lr_decay=0.9))
    batch = _batch(shape)
    with _recorded() as calls:
        _steps(m, ours, batch)
    _steps(ref, topt, batch)
    _assert_params_close(m, ref)
    stores = m.bert.encoder._stores
    flats = [s.flat.data_ptr() for s in stores]
    seg = [c for c in calls if c[0] in SEG_CALLS]
    assert sorted(c[1][0].data_ptr() for c in seg) == sorted(flats * 3), [c[0] for c in calls]
    assert not any(c[0] in ("adamw", "adamw_planes") for c in calls)
    layer_ptrs = _layer_ptrs(m)
    multi = [t.data_ptr() for c in calls if c[0] == "adamw_multi" for t in c[1][0]]
    assert multi and not (set(multi) & layer_ptrs)
    # 8 segments per layer: wqkv | bqkv | wo | bo ln1 | w1 | bi1 | w2 | bi2 ln2, weight decay on the matrices alone
    table = seg[0][1][4]
    assert len(table) == 8 and [wd for _, _, wd in table] == [1e-2, 0.0] * 4 and table[-1][0] == stores[0].flat.numel()
    if shape is WIDE:
        assert {c[0] for c in seg[len(flats):]} == {"adamw_planes_seg"}, [c[0] for c in seg]
    else:
        assert {c[0] for c in seg} == {"adamw_seg"}


def test_overlap_updates_split_layers_from_inside_backward():
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    outs = []
    for overlap in (False, True):
        m = _model()
        opt = AdamW(finetune_param_groups(m, 1e-3, layer_lr_decay=0.9), model=m, overlap=overlap)
        early = []
        with _recorded() as calls:
            losses = _steps(m, opt, _batch(), after_backward=lambda: early.append(set(opt._early)))
        outs.append((losses, m))
        if overlap:
            assert early == [{0, 1}] * 3, early  # both layers were updated before step() ran
            assert sum(c[0] in SEG_CALLS for c in calls) == 6
        else:
            assert early == [set()] * 3
    # the bounds of test_overlap_update_inside_backward_equals_the_plain_schedule
    torch.testing.assert_close(torch.tensor(outs[0][0]), torch.tensor(outs[1][0]), rtol=1e-5, atol=0)
    _assert_params_close(outs[0][1], outs[1][1], skip=("key.bias",))


def test_uniform_groups_call_no_segmented_binding_and_keep_their_bits():
    from mtvaf_amd.optim import AdamW, reference_param_groups
    finals = []
    for plans in (False, True):
        m = _model()
        opt = AdamW(reference_param_groups(m, 1e-3), model=m)
        if not plans:
            opt.SEGMENT_PLANS = False  # (test-only: the mapping of the commit before the segmented path)
            opt._map_layers()
        assert all(isinstance(g, dict) for g in opt._layer_group.values())
        with _recorded() as calls:
            _steps(m, opt, _batch())
        assert not any(c[0] in SEG_CALLS for c in calls) and sum(c[0] in ("adamw", "adamw_planes") for c in calls) == 6
        finals.append({n: p.detach().clone() for n, p in m.named_parameters()})
    for n, p in finals[0].items():
        assert _same(p, finals[1][n]), n


def test_a_layer_with_mixed_betas_goes_tensor_by_tensor_and_still_equals_torch():
    from mtvaf_amd.optim import AdamW

    def groups(model):
        named = [(n, p) for n, p in model.named_parameters() if "bert" in n or n.startswith("fc") or "crf" in n]
        return [{"params": [p for n, p in named if "bias" not in n], "betas": (0.9, 0.999)},
                {"params": [p for n, p in named if "bias" in n], "betas": (0.8, 0.99), "weight_decay": 0.0}]
    m = _model()
    ref = copy.deepcopy(m)
    ours, topt = AdamW(groups(m), lr=1e-3, model=m), torch.optim.AdamW(groups(ref), lr=1e-3)
    assert all(plan is None for plan in ours._layer_group.values())
    with _recorded() as calls:
        _steps(m, ours, _batch())
    _steps(ref, topt, _batch())
    assert {c[0] for c in calls} == {"adamw_multi"}
    assert _layer_ptrs(m) <= {t.data_ptr() for c in calls for t in c[1][0]}
    _assert_params_close(m, ref)


def test_a_scheduler_that_halves_the_lr_is_followed_by_the_segment_table():
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    m = _model()
    opt = AdamW(finetune_param_groups(m, 1e-3, layer_lr_decay=0.5), model=m)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s)
    with _recorded() as calls:
        _steps(m, opt, _batch(), steps=2, sched=sched)
    flat0 = m.bert.encoder._stores[0].flat.data_ptr()
    tables = [c[1][4] for c in calls if c[0] in SEG_CALLS and c[1][0].data_ptr() == flat0]
    assert len(tables) == 2 and len(tables[0]) == 8
    assert [lr for _, lr, _ in tables[0]] == [0.5e-3] * 8  # layer 0 of 2 at decay 0.5
    assert [lr for _, lr, _ in tables[1]] == [0.5 * lr for _, lr, _ in tables[0]]
    assert [(e, wd) for e, _, wd in tables[1]] == [(e, wd) for e, _, wd in tables[0]]


def test_clipping_with_split_groups_equals_torch_clip_then_adamw():
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    m = _model()
    ref = copy.deepcopy(m)
    batch = _batch()
    m(**batch).loss.backward()
    trained = [p for g in finetune_param_groups(m, 1e-3) for p in g["params"]]
    bound = 0.5 * float(torch.nn.utils.clip_grad_norm_([p for p in trained if p.grad is not None], 1e30))
    m.zero_grad(set_to_none=True)
    ours = AdamW(finetune_param_groups(m, 1e-3), model=m, max_grad_norm=bound)
    topt = torch.optim.AdamW(finetune_param_groups(ref, 1e-3))
    ref_trained = [p for g in topt.param_groups for p in g["params"]]
    with _recorded() as calls:
        _steps(m, ours, batch)
    _steps(ref, topt, batch, after_backward=lambda: torch.nn.utils.clip_grad_norm_([p for p in ref_trained if p.grad is not None], bound))
    seg = [c for c in calls if c[0] in SEG_CALLS]
    assert len(seg) == 6 and all(c[2].get("clip") is not None for c in seg)
    assert int(ours.skipped_steps) == 0 and float(ours.last_grad_norm) > 0
    _assert_params_close(m, ref)


def test_average_with_split_groups_leaves_the_run_alone_and_follows_the_weights():
    from mtvaf_amd.optim import AdamW, ema_decay_at, finetune_param_groups
    runs = []
    for decay in (0.0, 0.9):
        m = _model()
        opt = AdamW(finetune_param_groups(m, 1e-3), model=m, ema_decay=decay)
        snaps = []
        for _ in range(3):
            _steps(m, opt, _batch(), steps=1)
            snaps.append({n: p.detach().clone() for n, p in m.named_parameters()})
        runs.append((m, opt, snaps))
    for t in range(3):
        for n, p in runs[0][2][t].items():
            assert _same(p, runs[1][2][t][n]), (t, n)
    m, opt, snaps = runs[1]
    name = "bert.encoder.layer.1.output.LayerNorm.weight"  # (a no-decay tensor in the middle of a segmented buffer)
    for name in (name, "bert.encoder.layer.0.intermediate.dense.weight"):
        p = dict(m.named_parameters())[name]
        st = opt.state[p]
        assert int(st["ema_step"]) == 3 == int(st["step"])
        e = snaps[0][name].double()  # the first update makes the average the parameter
        for t in (1, 2):
            e = e + (1.0 - ema_decay_at(t, 0.9)) * (snaps[t][name].double() - e)
        torch.testing.assert_close(st["ema"].double(), e, rtol=1e-6, atol=1e-7)
        assert not _same(st["ema"], snaps[2][name])


@contextlib.contextmanager
def _compute(dtype):
    from mtvaf_amd import hip
    was = hip.COMPUTE
    hip.set_compute_dtype(dtype)
    try:
        yield
    finally:
        hip.set_compute_dtype(was)


def test_bf16_mode_keeps_the_shadow_equal_to_the_masters_under_split_groups():
    from mtvaf_amd import engine
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    with _compute("bf16"):
        m = _model(WIDE)
        opt = AdamW(finetune_param_groups(m, 1e-3), model=m)
        with _recorded() as calls:
            _steps(m, opt, _batch(WIDE))
        seg = [c for c in calls if c[0] in SEG_CALLS]
        assert len(seg) == 6 and {c[0] for c in seg} == {"adamw_seg"}
        assert all(c[2].get("p_bf16") is not None for c in seg[2:])  # (the first forward pass built the shadows)
        for store in m.bert.encoder._stores:
            sh = engine.shadow_for_update(store.weights)
            assert sh is not None and _same(sh, store.flat.to(torch.bfloat16))


def test_state_dict_round_trip_mid_run_continues_as_the_uninterrupted_run():
    from mtvaf_amd.optim import AdamW, finetune_param_groups
    batch = _batch()
    finals = []
    for resume in (False, True):
        m = _model()
        opt = AdamW(finetune_param_groups(m, 1e-3, layer_lr_decay=0.9), model=m)
        _steps(m, opt, batch, steps=2)
        if resume:
            sd_o, sd_m = copy.deepcopy(opt.state_dict()), copy.deepcopy(m.state_dict())
            m = _model()
            m.load_state_dict(sd_m)
            opt = AdamW(finetune_param_groups(m, 1e-3, layer_lr_decay=0.9), model=m)
            opt.load_state_dict(sd_o)
        with _recorded() as calls:
            _steps(m, opt, batch, steps=2)
        assert sum(c[0] in SEG_CALLS for c in calls) == 4
        w = m.bert.encoder.layer[1].intermediate.dense.weight
        assert int(opt.state[w]["step"]) == 4 and int(opt.state[m.bert.encoder.layer[1].output.LayerNorm.bias]["step"]) == 4
        finals.append(m)
    _assert_params_close(finals[1], finals[0])
