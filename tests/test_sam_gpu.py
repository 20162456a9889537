"""Sharpness-aware minimisation on the GPU: the mtvaf_sam_* kernels against the float64 restatement of tests/sam_cases.py, the
weight-image cache under AdamW.perturb() / step(), and SharpnessAware.step against the same step built from public pieces."""
import ctypes

import numpy as np
import pytest
import torch

import sam_cases as C
from optim_trace import recorded as _recorded
from test_ema_gpu import _batch, _mode, _model
from test_js_consistency_gpu import _batch as span_batch, _build as span_build
from test_ops_gpu import DEV, hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
IDS = [c["id"] for c in C.CASES]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _finalize(hip, gs, rho=C.RHO):
    partials = hip.grad_sqnorm(gs)
    state = torch.full((4,), 9.0, device=DEV)
    skipped = torch.zeros((), dtype=torch.int32, device=DEV)
    hip.sam_finalize(partials, rho, state, skipped)
    return partials, state, skipped


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_finalize_and_perturb_hold_the_contract(hip, case):
    p, g = C.make_inputs(case["n"], case["kind"])
    pd, gd = p.to(DEV), g.to(DEV)
    backup = torch.full_like(pd, 7.0)
    partials, state, skipped = _finalize(hip, [gd])
    hip.sam_perturb(pd, gd, backup, state)
    torch.cuda.synchronize()
    st = state.cpu()
    assert partials.numel() == -(-case["n"] // C.CHUNK) and float(st[3]) == 0.0
    assert _same(backup.cpu(), p)  # backup is the old p whatever the norm was
    dev_norm64 = C.ordered_norm64(partials.cpu().tolist())
    ref = C.reference([p], [g], C.RHO, scale=float(st[1]))
    print(f"{case['id']}: norm {float(st[0])!r} (float64 {ref['norm']!r}), scale {float(st[1])!r}, finite {float(st[2])}")
    if case["kind"] in ("overflow32", "inf", "nan"):
        assert not C.fits32(dev_norm64) and not ref["finite"]
        assert float(st[1]) == 0.0 and float(st[2]) == 0.0 and int(skipped) == 1 and not np.isfinite(float(st[0]))
        assert _same(pd.cpu(), p)  # p keeps its bits: no arithmetic touched it
        return
    assert float(st[2]) == 1.0 and int(skipped) == 0
    norm_ulp = float(C.ulp32(torch.tensor([ref["norm"]], dtype=torch.float64)))
    assert abs(float(st[0].double()) - ref["norm"]) <= norm_ulp, (float(st[0]), ref["norm"])
    want_scale = C.scale32(C.RHO, dev_norm64)
    assert st[1].numpy().view(np.int32) == want_scale.view(np.int32), (float(st[1]), float(want_scale))
    excess = C.half_ulp_excess(pd, ref["p_new"][0])
    print(f"  |p_new - (p + scale g)| in half ulps of p_new: {excess:.4f}")
    assert excess <= 1.0
    if case["kind"] == "zero":
        assert float(st[0]) == 0.0 and _same(pd.cpu(), p)  # scale * 0 = 0
    elif case["kind"] != "scaled-down":  # (a norm below the 1e-12 of the denominator gives a step shorter than rho: it may round away)
        assert not _same(pd.cpu(), p)


# one buffer: the smallest legal matrix, a gap that belongs to no matrix, a matrix of three rows, one that spans several blocks, a tail
MATS = [(0, 1, 32), (44, 3, 64), (240, 40, 96)]
N_BUF = 240 + 40 * 96 + 8


def _images(hip, flat):
    """-> the plane images of MATS as hip.split_planes_blocked builds them from `flat`"""
    out = []
    for b, r, c in MATS:
        img = torch.empty(6 * r * c, dtype=torch.uint8, device=DEV)
        hip.split_planes_blocked(flat[b:b + r * c].view(r, c).contiguous(), img)
        out.append(img)
    return out


def _shadow(hip, flat):
    out = torch.empty(flat.numel(), dtype=torch.bfloat16, device=DEV)
    hip.cast_bf16(flat.view(1, -1), out=out.view(1, -1))
    return out


def test_three_forms_give_the_same_bits_and_maintain_shadow_and_images(hip):
    p, g = C.make_inputs(N_BUF, "randn", seed=1)
    gd = g.to(DEV)
    _, state, _ = _finalize(hip, [gd])
    # plain, with the bf16 shadow
    p1, b1 = p.to(DEV), torch.zeros(N_BUF, device=DEV)
    sh = torch.zeros(N_BUF, dtype=torch.bfloat16, device=DEV)
    hip.sam_perturb(p1, gd, b1, state, p_bf16=sh)
    # planes
    p2, b2 = p.to(DEV), torch.zeros(N_BUF, device=DEV)
    imgs = [torch.full((6 * r * c,), 0x5A, dtype=torch.uint8, device=DEV) for _, r, c in MATS]
    segs = [(b, r, c, im) for (b, r, c), im in zip(MATS, imgs)]
    hip.sam_perturb_planes(p2, gd, b2, state, segs)
    # multi: the buffer as two views, the second 4 bytes off a 16-byte boundary
    p3, b3 = p.to(DEV), torch.zeros(N_BUF, device=DEV)
    cut = 5
    hip.sam_perturb_multi([p3[:cut], p3[cut:]], [gd[:cut], gd[cut:]], [b3[:cut], b3[cut:]], state)
    torch.cuda.synchronize()
    assert _same(p1, p2) and _same(p1, p3) and not _same(p1, p.to(DEV))
    for b in (b1, b2, b3):
        assert _same(b.cpu(), p)
    assert torch.equal(sh.view(torch.int16), _shadow(hip, p1).view(torch.int16))
    for got, want in zip(imgs, _images(hip, p2)):
        assert torch.equal(got, want)
    # the way back, each form: the original bits, shadow and images of the restored values
    hip.sam_restore(p1, b1, p_bf16=sh)
    hip.sam_restore_planes(p2, b2, segs)
    hip.sam_restore_multi([p3[:cut], p3[cut:]], [b3[:cut], b3[cut:]])
    torch.cuda.synchronize()
    for q in (p1, p2, p3):
        assert _same(q.cpu(), p)
    assert torch.equal(sh.view(torch.int16), _shadow(hip, p1).view(torch.int16))
    for got, want in zip(imgs, _images(hip, p2)):
        assert torch.equal(got, want)
    # a non-finite state: p keeps its bits, and shadow and images are written from it
    bad = torch.tensor([float("inf"), 0.0, 0.0, 0.0], device=DEV)
    sh.zero_()
    for im in imgs:
        im.fill_(0x5A)
    b1.zero_(); b2.zero_()
    gnan = torch.full_like(gd, float("nan"))
    hip.sam_perturb(p1, gnan, b1, bad, p_bf16=sh)
    hip.sam_perturb_planes(p2, gnan, b2, bad, segs)
    torch.cuda.synchronize()
    assert _same(p1.cpu(), p) and _same(p2.cpu(), p) and _same(b1.cpu(), p) and _same(b2.cpu(), p)
    assert torch.equal(sh.view(torch.int16), _shadow(hip, p1).view(torch.int16))
    for got, want in zip(imgs, _images(hip, p2)):
        assert torch.equal(got, want)


def test_multi_tensor_form_across_the_launch_boundary_and_off_alignment(hip):
    """C.MULTI (every edge length, some bases 4 bytes off) and 45 short tensors behind them: 54 tensors, two launches."""
    lens = list(C.MULTI) + [(3, i % 2) for i in range(45)]
    ps, gs, p0 = [], [], []
    for i, (n, off) in enumerate(lens):
        p, g = C.make_inputs(n, "randn", seed=10 + i)
        p0.append(p)
        pb, gb = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
        pb[off:off + n].copy_(p); gb[off:off + n].copy_(g)
        ps.append(pb[off:off + n]); gs.append(gb[off:off + n])
        assert ps[-1].data_ptr() % 16 == 4 * off
    partials, state, skipped = _finalize(hip, gs)
    assert partials.numel() == sum(-(-n // C.CHUNK) for n, _ in lens)
    ref = [q.clone() for q in ps]
    bs_one = [torch.zeros_like(q) for q in ps]
    for q, g, b in zip(ref, gs, bs_one):
        hip.sam_perturb(q, g, b, state)
    bs = [torch.zeros_like(q) for q in ps]
    hip.sam_perturb_multi(ps, gs, bs, state)
    torch.cuda.synchronize()
    st = state.cpu()
    want = C.reference(p0, [g.cpu() for g in gs], C.RHO, scale=float(st[1]))
    assert st[1].numpy().view(np.int32) == C.scale32(C.RHO, C.ordered_norm64(partials.cpu().tolist())).view(np.int32)
    for i, (q, r, b) in enumerate(zip(ps, ref, bs)):
        assert _same(q, r) and _same(b.cpu(), p0[i]), i
        assert C.half_ulp_excess(q, want["p_new"][i]) <= 1.0, i
    hip.sam_restore_multi(ps, bs)
    torch.cuda.synchronize()
    for q, p in zip(ps, p0):
        assert _same(q.cpu(), p)


def test_bad_arguments_return_err_arg_and_write_nothing(hip):
    L, st = hip.lib(), hip._st()
    ARG = -3
    n = 64
    buf = torch.arange(4 * n, dtype=torch.float32, device=DEV)
    keep = buf.clone()
    p, g, b = buf[:n], buf[n:2 * n], buf[2 * n:3 * n]
    state = torch.tensor([1.0, 0.5, 1.0, 0.0], device=DEV)
    img = torch.zeros(6 * 32, dtype=torch.uint8, device=DEV)
    P, G, B, S = p.data_ptr(), g.data_ptr(), b.data_ptr(), state.data_ptr()
    assert L.mtvaf_sam_perturb(None, G, B, n, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, None, B, n, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, G, None, n, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, G, B, n, None, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, G, B, 0, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, G, B, -4, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P, G, P + 4 * (n - 1), n, S, None, st) == ARG   # backup overlaps p
    assert L.mtvaf_sam_perturb(P, G, P, n, S, None, st) == ARG
    assert L.mtvaf_sam_perturb(P + 2, G, B, n - 1, S, None, st) == ARG           # 2 bytes off
    assert L.mtvaf_sam_restore(P, P + 4, n, None, st) == ARG
    assert L.mtvaf_sam_restore(P, None, n, None, st) == ARG
    assert L.mtvaf_sam_restore(P, B, 0, None, st) == ARG
    one = lambda x: (ctypes.c_void_p * 1)(x)
    beg, rows, cols = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(32)
    im = one(img.data_ptr())
    assert L.mtvaf_sam_perturb_planes(P, G, B, n - 1, S, 1, beg, rows, cols, im, st) == ARG      # n % 4
    assert L.mtvaf_sam_perturb_planes(P + 4, G, B, n - 4, S, 1, beg, rows, cols, im, st) == ARG  # p 4 bytes off 16
    assert L.mtvaf_sam_perturb_planes(P, G, P + 16, n, S, 1, beg, rows, cols, im, st) == ARG
    assert L.mtvaf_sam_perturb_planes(P, G, B, n, S, 5, beg, rows, cols, im, st) == ARG          # nseg > 4, as mtvaf_adamw_planes
    assert L.mtvaf_sam_perturb_planes(P, G, B, n, S, 1, beg, rows, (ctypes.c_int * 1)(48), im, st) == -1  # cols % 32: its ERR_SHAPE
    assert L.mtvaf_sam_restore_planes(P, B, n, 1, beg, rows, cols, None, st) == ARG
    assert L.mtvaf_sam_restore_planes(P, P, n, 1, beg, rows, cols, im, st) == ARG
    two = lambda x, y: (ctypes.c_void_p * 2)(x, y)
    n2 = (ctypes.c_long * 2)(8, 8)
    # a good tensor in front of a bad one: the whole call is refused before the first launch
    assert L.mtvaf_sam_perturb_multi(2, two(P, P + 64), two(G, G + 64), two(B, P + 64), n2, S, st) == ARG
    assert L.mtvaf_sam_perturb_multi(2, two(P, P + 64), two(G, None), two(B, B + 64), n2, S, st) == ARG
    assert L.mtvaf_sam_perturb_multi(-1, two(P, P + 64), two(G, G + 64), two(B, B + 64), n2, S, st) == ARG
    assert L.mtvaf_sam_restore_multi(2, two(P, P + 64), two(B, P + 80), n2, st) == ARG
    assert L.mtvaf_sam_restore_multi(1, None, one(B), n2, st) == ARG
    part = torch.ones(2, dtype=torch.float64, device=DEV)
    assert L.mtvaf_sam_finalize(part.data_ptr(), 2, 0.05, None, None, st) == ARG
    assert L.mtvaf_sam_finalize(None, 2, 0.05, S, None, st) == ARG
    assert L.mtvaf_sam_finalize(part.data_ptr(), -1, 0.05, S, None, st) == ARG
    assert L.mtvaf_sam_finalize(part.data_ptr(), 2, -1.0, S, None, st) == ARG
    assert L.mtvaf_sam_finalize(part.data_ptr(), 2, float("nan"), S, None, st) == ARG
    assert L.mtvaf_sam_finalize(part.data_ptr(), 2, 0.05, S + 4, None, st) == ARG
    torch.cuda.synchronize()
    assert _same(buf, keep) and float(state[1]) == 0.5 and int(img.sum()) == 0
    assert L.mtvaf_sam_perturb_multi(0, None, None, None, None, S, st) == 0
    assert L.mtvaf_sam_restore_multi(0, None, None, None, st) == 0


# ---- 2. the optimizer and the weight-image cache ---------------------------------------------------------------------------
def _loaded_copy(m):
    """A fresh model of the same architecture whose parameters were loaded through load_state_dict: its images are built anew."""
    m2, _ = _model()
    m2.load_state_dict(m.state_dict())
    return m2


def _eval_forward(m, batch):
    with torch.no_grad():
        out = m(**batch)
    lg = out.logits
    lg = lg.detach().cpu().tolist() if torch.is_tensor(lg) else [[int(t) for t in row] for row in lg]  # (decoded tags: ragged)
    return out.loss.detach().clone(), lg


def _on_the_image_path(m, mode):
    from mtvaf_amd import engine
    ws = [st.weights for st in m.bert.encoder._stores]
    if mode == "planes":
        return engine.LAST_PACK is not None and engine.LAST_PACK.Mp >= engine.F32_PLANES_MIN_ROWS and all(w._pl is not None for w in ws)
    return all(w._h is not None for w in ws)


@pytest.mark.parametrize("mode", ["planes", "bf16"])
def test_forward_after_perturb_and_after_step_reads_the_weights_that_are_there(mode):
    """The stale-image trap: the GEMMs read cached images of the weights, not the weights."""
    from mtvaf_amd.optim import AdamW
    with _mode(mode):
        m, cfg = _model()
        batch = _batch(cfg)
        opt = AdamW(m.parameters(), lr=1e-3, model=m, sam_rho=C.RHO)
        clean = _eval_forward(m, batch)
        m(**batch).loss.backward()
        assert _on_the_image_path(m, mode)
        w0 = m.bert.encoder.layer[1].intermediate.dense.weight.detach().clone()
        opt.perturb()
        assert opt.sam_perturbed and all(p.grad is None for p in m.parameters())
        assert not _same(m.bert.encoder.layer[1].intermediate.dense.weight, w0) and float(opt.last_sam_norm) > 0 and int(opt.sam_skipped) == 0
        got = _eval_forward(m, batch)
        assert _on_the_image_path(m, mode)
        want = _eval_forward(_loaded_copy(m), batch)
        assert torch.equal(got[0], want[0]) and got[1] == want[1]
        assert not torch.equal(got[0], clean[0])  # (the comparison can tell the two sets of weights apart)
        m(**batch).loss.backward()
        opt.step()
        opt.zero_grad()
        assert not opt.sam_perturbed
        got = _eval_forward(m, batch)
        assert _on_the_image_path(m, mode)
        want = _eval_forward(_loaded_copy(m), batch)
        assert torch.equal(got[0], want[0]) and got[1] == want[1]
        # no key of the checkpoint knows about SAM, and no backup is in it
        plain = AdamW(_model()[0].parameters(), lr=1e-3)
        sd = opt.state_dict()
        assert set(sd) == set(plain.state_dict()) and set(sd["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
        assert all(set(s) <= {"exp_avg", "exp_avg_sq", "step"} for s in sd["state"].values())


def _fma32(p, g, scale):
    """fmaf(scale, g, p) on the host: the product is exact in 48 bits, the sum is formed with a 64-bit significand and rounded to
    fp32 (a double rounding that differs from one rounding for about one value in 2^40)"""
    pl, gl = p.detach().cpu().numpy().astype(np.longdouble), g.detach().cpu().numpy().astype(np.longdouble)
    return torch.from_numpy((pl + np.longdouble(scale) * gl).astype(np.float32))


def _tagger():
    m, cfg = _model()
    return m, _batch(cfg)


def _span():
    return span_build(False)[0].eval(), span_batch(False)


def _groups(m, segmented):
    from mtvaf_amd.optim import finetune_param_groups
    if segmented:
        return finetune_param_groups(m, 1e-3, use_prefix=False)
    return [{"params": list(m.parameters())}]


EQUIV = {"tagger": (_tagger, False, {}), "tagger-segmented": (_tagger, True, {}), "tagger-ema": (_tagger, False, dict(ema_decay=0.9)),
         "tagger-clip": (_tagger, False, dict(max_grad_norm=0.05)), "span": (_span, False, {}), "span-segmented": (_span, True, {})}


@pytest.mark.parametrize("which", sorted(EQUIV))
def test_step_equals_the_sequence_built_from_public_pieces(which):
    from mtvaf_amd.optim import AdamW
    from mtvaf_amd.sam import SharpnessAware
    build, segmented, kw = EQUIV[which]
    m, batch = build()
    opt = AdamW(_groups(m, segmented), lr=1e-3, model=m, sam_rho=C.RHO, **kw)
    res = SharpnessAware(m, opt).step(**batch)
    scale = float(opt._sam_state[1])
    assert scale > 0 and not opt.sam_perturbed and float(res["grad_norm"]) == float(opt.last_sam_norm)
    assert float(res["sam_loss"]) != float(res["loss"]) and all(p.grad is None for p in m.parameters())
    if segmented:
        assert any(isinstance(plan, list) for plan in opt._layer_group.values())
    # by hand: first backward, perturbed values on the host, a copy's backward, its gradients under a plain step of the original
    mb, _ = build()
    optb = AdamW(_groups(mb, segmented), lr=1e-3, model=mb, **kw)
    out1 = mb(**batch)
    out1.loss.backward()
    assert torch.equal(out1.loss.detach(), res["loss"])
    mc, _ = build()
    named_b = dict(mb.named_parameters())
    sd = {k: v.clone() for k, v in mb.state_dict().items()}
    for n, p in named_b.items():
        if p.grad is not None:
            sd[n] = _fma32(p, p.grad, np.float32(scale)).view(p.shape).to(DEV)
    mc.load_state_dict(sd)
    out2 = mc(**batch)
    out2.loss.backward()
    assert torch.equal(out2.loss.detach(), res["sam_loss"])
    with torch.no_grad():
        for n, p in mc.named_parameters():
            if p.grad is not None:
                named_b[n].grad.copy_(p.grad)  # (in place: the gradients stay where the first pass put them)
    optb.step()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    checked = 0
    for n, pb in named_b.items():
        assert _same(named[n], pb), n
        sa, sb = opt.state.get(named[n], {}), optb.state.get(pb, {})
        assert set(sa) == set(sb), n
        for k in ("exp_avg", "exp_avg_sq", "ema"):
            if k in sb:
                assert _same(sa[k], sb[k]), (n, k)
                checked += 1
    assert checked >= (3 if "ema_decay" in kw else 2) * 32
    if "max_grad_norm" in kw:
        assert float(optb.last_grad_norm) > kw["max_grad_norm"] and _same(opt.last_grad_norm, optb.last_grad_norm)  # (it did clip)


@pytest.mark.parametrize("mode", ["planes", "bf16"])
def test_a_step_the_clipping_drops_leaves_weights_and_images_of_before_perturb(mode):
    from mtvaf_amd.optim import AdamW
    with _mode(mode):
        m, cfg = _model()
        batch = _batch(cfg)
        opt = AdamW(m.parameters(), lr=1e-3, model=m, sam_rho=C.RHO, max_grad_norm=1.0, ema_decay=0.9)
        for _ in range(1):  # one good step: moments and averages exist
            m(**batch).loss.backward(); opt.perturb(); m(**batch).loss.backward(); opt.step(); opt.zero_grad()
        assert int(opt.skipped_steps) == 0
        before_fwd = _eval_forward(m, batch)
        snap = {n: (p.detach().clone(), {k: v.detach().clone() for k, v in opt.state[p].items() if torch.is_tensor(v) and v.dim() > 0})
                for n, p in m.named_parameters() if p in opt.state}
        m(**batch).loss.backward()
        opt.perturb()
        m(**batch).loss.backward()
        assert _on_the_image_path(m, mode)
        m.bert.encoder.layer[0].output.dense.weight.grad[3, 5] = float("inf")  # a value, not a fault
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        assert int(opt.skipped_steps) == 1 and not opt.sam_perturbed
        for n, p in m.named_parameters():
            if n in snap:
                assert _same(p, snap[n][0]), n
                for k, v in snap[n][1].items():
                    assert _same(opt.state[p][k], v), (n, k)
        assert "ema" in snap["fc.weight"][1] and "exp_avg" in snap["bert.encoder.layer.0.output.dense.weight"][1]
        after_fwd = _eval_forward(m, batch)
        assert _on_the_image_path(m, mode)
        assert torch.equal(after_fwd[0], before_fwd[0]) and after_fwd[1] == before_fwd[1]


def test_a_nonfinite_first_gradient_leaves_the_weights_alone_and_is_counted():
    from mtvaf_amd.optim import AdamW
    m, cfg = _model()
    batch = _batch(cfg)
    opt = AdamW(m.parameters(), lr=1e-3, model=m, sam_rho=C.RHO)
    m(**batch).loss.backward()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.fc.weight.grad[0, 0] = float("nan")
    opt.perturb()
    torch.cuda.synchronize()
    assert int(opt.sam_skipped) == 1 and opt.sam_perturbed
    for n, p in m.named_parameters():
        assert _same(p, before[n]), n
    opt.unperturb()
    assert not opt.sam_perturbed
    for n, p in m.named_parameters():
        assert _same(p, before[n]), n


def test_refusals():
    from mtvaf_amd.graph import GraphedTrainStep
    from mtvaf_amd.optim import AdamW, build_optimizer, schedule_table
    from mtvaf_amd.sam import SharpnessAware
    m, cfg = _model()
    batch = _batch(cfg)
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="overlap=False"):
        AdamW(ps, model=m, sam_rho=0.05, overlap=True)
    with pytest.raises(ValueError, match="accumulation_steps"):
        AdamW(ps, model=m, sam_rho=0.05, accumulation_steps=2)
    with pytest.raises(ValueError, match="device_schedule"):
        AdamW(ps, model=m, sam_rho=0.05, device_schedule=schedule_table(lambda t: 1.0, 4))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sam_rho"):
            AdamW(ps, sam_rho=bad)

    class GradSync:  # (what attach sees of one: its world size)
        world, force, accumulation_steps = 2, False, 1

        def adopt_optimizer(self, opt):
            pass
    with pytest.raises(RuntimeError, match="several ranks"):
        AdamW(ps, model=m, sam_rho=0.05, grad_sync=GradSync())
    plain = AdamW(ps, model=m)
    with pytest.raises(RuntimeError, match="sam_rho=0"):
        plain.perturb()
    with pytest.raises(ValueError, match="sam_rho > 0"):
        SharpnessAware(m, plain)
    sched = AdamW(ps, model=m, device_schedule=schedule_table(lambda t: 1.0, 4))
    sched.sam_rho = 0.05  # (set behind the constructor's back: the capture still refuses it)
    with pytest.raises(RuntimeError, match="not captured"):
        GraphedTrainStep(m, batch, optimizer=sched)
    opt = AdamW(ps, lr=1e-3, model=m, sam_rho=0.05, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no parameter has a gradient"):
        opt.perturb()
    m(**batch).loss.backward()
    opt.step()  # step() without perturb() is a plain step
    opt.zero_grad()
    m(**batch).loss.backward()
    opt.swap_ema()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.perturb()
    opt.swap_ema()
    opt.perturb()
    with pytest.raises(RuntimeError, match="twice"):
        opt.perturb()
    with pytest.raises(RuntimeError, match="perturbed"):
        opt.load_state_dict(opt.state_dict())
    opt.unperturb()
    opt.load_state_dict(opt.state_dict())
    args = type("A", (), dict(lr=1e-3, sam_rho=0.05, warmup_ratio=0.1))()
    built, _ = build_optimizer(m, args, 10)
    assert built.sam_rho == 0.05 and built.overlap is False
    args.gradient_accumulation_steps = 2
    with pytest.raises(ValueError, match="sam_rho"):
        build_optimizer(m, args, 10)
    args.gradient_accumulation_steps, args.sam_rho = 1, 0.0
    assert build_optimizer(m, args, 10)[0].sam_rho == 0.0


def test_default_is_the_step_it_was(hip):
    from mtvaf_amd.optim import AdamW
    seqs, sds = [], []
    for kw in ({}, dict(sam_rho=0.0)):
        m, cfg = _model()
        batch = _batch(cfg)
        opt = AdamW(m.parameters(), lr=1e-3, model=m, max_grad_norm=1.0, **kw)
        with _recorded(hip) as calls:
            for _ in range(2):
                m(**batch).loss.backward()
                opt.step()
                opt.zero_grad()
        seqs.append(list(calls))
        sds.append(opt.state_dict())
        assert opt.sam_rho == 0.0 and opt._sam_state is None and not opt._sam_backup and opt.sam_skipped is None
        assert "sam_rho" not in opt.defaults and all("sam_rho" not in g for g in opt.param_groups)
    assert seqs[0] == seqs[1] and seqs[0] and not any(c.startswith("sam_") for c in seqs[0])
    assert seqs[0].count("grad_sqnorm") == 2 and any(c.startswith("adamw") for c in seqs[0])
    assert set(sds[0]) == set(sds[1]) and [set(g) for g in sds[0]["param_groups"]] == [set(g) for g in sds[1]["param_groups"]]
