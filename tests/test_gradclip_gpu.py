"""Gradient clipping inside the AdamW step on the MI355X (csrc/gradnorm.hip, the *_dev kernels of csrc/optim.hip,
mtvaf_amd.optim.AdamW(max_grad_norm=...)) against the float64 restatement of gradclip_cases.py and against
torch.nn.utils.clip_grad_norm_ in front of the unclipped optimizer."""
import copy
import math

import numpy as np
import pytest
import torch

import gradclip_cases as GC
import params as P
from test_model_gpu import DEV, LABELS, _prompt_inputs, hf_config, make_args

pytestmark = pytest.mark.gpu

HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2)  # lr, beta1, beta2, eps, weight decay


# ---- the kernels --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    """One call of the norm kernel over the case list + one finalize: shared, read-only."""
    from mtvaf_amd import hip
    cpu = GC.norm_tensors()
    dev = []
    for t in cpu:  # the view stays a view: its base lands on a 16-byte boundary, the view 4 bytes behind it
        dev.append(t._base.to(DEV)[1:] if t._base is not None else t.to(DEV))
    part = hip.grad_sqnorm(dev).clone()
    state = torch.zeros(4, device=DEV)
    skipped = torch.zeros((), dtype=torch.int32, device=DEV)
    hip.grad_clip_finalize(part, 0.0, state, skipped)
    torch.cuda.synchronize()
    return dict(cpu=cpu, dev=dev, part=part, state=state.cpu(), skipped=int(skipped), want=GC.global_norm(cpu))


def test_norm_equals_the_float64_norm_rounded_once(measured):
    from mtvaf_amd import hip
    dev, part = measured["dev"], measured["part"]
    assert any(t.data_ptr() % 16 == 4 for t in dev) and len(dev) > 48
    assert part.numel() == GC.expected_slots([t.numel() for t in dev]) == hip.grad_sqnorm_slots(dev)
    want = float(np.float32(measured["want"]))
    got = float(measured["state"][0])
    print(f"norm {got!r} float64 {measured['want']!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 2.0 ** -23 * want
    assert measured["state"].tolist()[1:] == [1.0, 1.0, 0.0] and measured["skipped"] == 0
    # each tensor's partial sums are its own sum of squares (slot order: tensor after tensor)
    s = 0
    for t, c in zip(dev, measured["cpu"]):
        k = (t.numel() + GC.CHUNK - 1) // GC.CHUNK
        one = float(part[s:s + k].sum())
        ref = float(np.sum(np.square(c.double().numpy())))
        assert abs(one - ref) <= 1e-12 * ref, (t.numel(), one, ref)
        s += k
    # same inputs, same bits
    again = hip.grad_sqnorm(dev)
    state2 = torch.zeros(4, device=DEV)
    hip.grad_clip_finalize(again, 0.0, state2)
    assert torch.equal(again, part) and torch.equal(state2.cpu(), measured["state"])


def test_one_huge_gradient_gives_a_finite_norm():
    from mtvaf_amd import hip
    g = torch.zeros(GC.CHUNK + 9, device=DEV)
    g[GC.CHUNK + 2] = 1e20  # squares to 1e40: beyond fp32, nothing to a double
    state = torch.zeros(4, device=DEV)
    skipped = torch.zeros((), dtype=torch.int32, device=DEV)
    hip.grad_clip_finalize(hip.grad_sqnorm([g]), 1.0, state, skipped)
    norm, coef, finite, _ = state.tolist()
    assert finite == 1.0 and int(skipped) == 0
    assert abs(norm - 1e20) <= 2.0 ** -23 * 1e20
    assert abs(coef - 1e-20) <= 2.0 ** -22 * 1e-20


def test_finalize_rule(measured):
    from mtvaf_amd import hip
    part = measured["part"]
    N = float(measured["state"][0])
    state = torch.zeros(4, device=DEV)
    hip.grad_clip_finalize(part, N / 4, state)
    norm, coef, finite, _ = state.tolist()
    want = float(np.float32(float(np.float32(N / 4)) / (N + 1e-6)))  # (max_norm crosses the C ABI as a float)
    print(f"coef {coef!r} want {want!r}")
    assert norm == N and finite == 1.0 and abs(coef - want) <= 2.0 ** -22 * want
    hip.grad_clip_finalize(part, 4 * N, state)
    assert state.tolist() == [N, 1.0, 1.0, 0.0]
    state.fill_(7.0)
    hip.grad_clip_finalize(part, 0.0, state)
    assert state.tolist() == [N, 1.0, 1.0, 0.0]


def test_nonfinite_partials_set_the_skip_state_and_count():
    from mtvaf_amd import hip
    for bad in (float("inf"), float("nan")):
        g = torch.randn(300, device=DEV)
        g[17] = bad
        state = torch.zeros(4, device=DEV)
        skipped = torch.zeros((), dtype=torch.int32, device=DEV)
        part = hip.grad_sqnorm([g])
        hip.grad_clip_finalize(part, 1.0, state, skipped)
        norm, coef, finite, _ = state.tolist()
        assert not math.isfinite(norm) and coef == 0.0 and finite == 0.0 and int(skipped) == 1
        hip.grad_clip_finalize(part, 1.0, state, skipped, skip_nonfinite=False)  # torch's rule: inf -> 0, NaN -> NaN; no skip
        norm, coef, finite, _ = state.tolist()
        assert finite == 1.0 and int(skipped) == 1
        assert (coef == 0.0) if math.isinf(bad) else math.isnan(coef)


def _flat_case():
    """A flat buffer of 2 x (64 x 32) floats holding two matrices with plane images, and a 1027-element tensor whose four bases
    are 4-byte aligned only (the scalar body)."""
    torch.manual_seed(3)
    n = 2 * 64 * 32
    flat = [torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 0.1, torch.randn(n, device=DEV) * 0.01,
            torch.rand(n, device=DEV) * 0.01]
    segs = lambda: [(0, 64, 32, torch.full((6 * 64 * 32,), 0x7f, dtype=torch.uint8, device=DEV)),
                    (64 * 32, 64, 32, torch.full((6 * 64 * 32,), 0x7f, dtype=torch.uint8, device=DEV))]
    odd = [torch.randn(1028, device=DEV), torch.randn(1028, device=DEV) * 0.1, torch.randn(1028, device=DEV) * 0.01,
           torch.rand(1028, device=DEV) * 0.01]
    return flat, segs, odd


def _run_all(clip, flat, segs, odd, step=3):
    """The three entry points on fresh copies -> every tensor they write."""
    from mtvaf_amd import hip
    out = []
    for base in (flat, odd):
        p, g, m, v = (t.clone()[1:] if base is odd else t.clone() for t in base)
        assert (p.data_ptr() % 16 == 4) == (base is odd)
        sh = torch.full((p.numel(),), 7.0, dtype=torch.bfloat16, device=DEV)
        hip.adamw(p, g, m, v, *HYPER, step, p_bf16=sh, clip=clip)
        out += [p, m, v, sh]
        p, g, m, v = (t.clone()[1:] if base is odd else t.clone() for t in base)
        p2, g2, m2, v2 = (t.clone() for t in flat)
        hip.adamw_multi([p, p2], [g, g2], [m, m2], [v, v2], *HYPER, step, clip=clip)
        out += [p, m, v, p2, m2, v2]
    p, g, m, v = (t.clone() for t in flat)
    sg = segs()
    hip.adamw_planes(p, g, m, v, *HYPER, step, sg, clip=clip)
    out += [p, m, v, sg[0][3], sg[1][3]]
    return out


def test_dev_forms_equal_the_host_scalar_forms_bit_for_bit_when_not_clipping():
    from mtvaf_amd import hip
    flat, segs, odd = _flat_case()
    state = torch.zeros(4, device=DEV)
    hip.grad_clip_finalize(hip.grad_sqnorm([flat[1], odd[1][1:]]), 0.0, state)  # coef == 1 from the kernel itself
    assert state.tolist()[1:3] == [1.0, 1.0]
    plain = _run_all(None, flat, segs, odd)
    dev = _run_all(state, flat, segs, odd)
    assert len(plain) == len(dev) == 25
    for i, (a, b) in enumerate(zip(plain, dev)):
        assert torch.equal(a, b), i
    assert not torch.equal(plain[0], flat[0]) and not (plain[-1] == 0x7f).all()  # (and the calls did update)
    # finite == 0: nothing at all is written
    state[1:3] = 0.0
    frozen = _run_all(state, flat, segs, odd)
    for i in (0, 4, 10, 14, 20):  # p of every call
        assert torch.equal(frozen[i], (flat if i in (0, 4, 20) else odd)[0][(0 if i in (0, 4, 20) else 1):]), i
    assert (frozen[3] == 7.0).all() and (frozen[-1] == 0x7f).all() and (frozen[-2] == 0x7f).all()
    assert torch.equal(frozen[1], flat[2]) and torch.equal(frozen[2], flat[3])


def test_the_coefficient_reaches_the_update():
    """One step from zero moments: m = (1 - beta1) * (g * coef).  (p after one Adam step does not depend on the gradient's scale: a
    test on p would pass with any coefficient.)"""
    from mtvaf_amd import hip
    flat, segs, odd = _flat_case()
    for t in (flat, odd):
        t[2].zero_()
        t[3].zero_()
    state = torch.zeros(4, device=DEV)
    part = hip.grad_sqnorm([flat[1]])
    hip.grad_clip_finalize(part, 0.0, state)
    hip.grad_clip_finalize(part, float(state[0]) / 4, state)
    coef = float(state[1])
    assert abs(coef - 0.25) < 1e-6
    out = _run_all(state, flat, segs, odd, step=1)
    want_flat = (1.0 - 0.9) * (flat[1].double() * coef)
    want_odd = (1.0 - 0.9) * (odd[1][1:].double() * coef)
    # (index of m in _run_all's output: adamw, multi (odd or flat, then flat), ..., planes)
    for i, want in ((1, want_flat), (5, want_flat), (8, want_flat), (11, want_odd), (15, want_odd), (18, want_flat), (21, want_flat)):
        err = ((out[i].double() - want).abs() / want.abs().clamp_min(1e-300)).max()
        print(f"m[{i}] max rel err {float(err):.3e}")
        torch.testing.assert_close(out[i].double(), want, rtol=2.0 ** -22, atol=0, msg=str(i))


# ---- the optimizer ------------------------------------------------------------------------------------------------------
def _model(layers=2):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=layers, max_pos=64)
    args = make_args(alpha=0.0)
    args.bert_config = hf_config(cfg, dropout=0.0)
    torch.manual_seed(11)
    return TVNetSAModel2(LABELS, None, args).to(DEV), cfg


def _batch(cfg, B=16, S=64, seed=5):
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, seed, B, S, lo_id=5))
    feats, aux, _ = (t.to(DEV) for t in _prompt_inputs(seed + 1, B, 3))
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats, aux_imgs=aux)


def test_optimizer_follows_the_float64_restatement_and_clipping_changes_the_trajectory():
    """The tiny model's parameters as a plain list in the reference's three groups (no encoder attached: everything goes through the
    multi-tensor kernel, more than 48 tensors in the first group), fixed gradients scaled 1, 10, 0.1."""
    from mtvaf_amd.optim import AdamW, reference_param_groups
    m, _ = _model(layers=3)
    gen = torch.Generator().manual_seed(21)
    groups = reference_param_groups(m, 3e-3)
    plist = [p for g in groups for p in g["params"]]
    assert 55 <= len(plist) <= 120 and len(groups[0]["params"]) > 48 and len(groups[2]["params"]) > 0, [len(g["params"]) for g in groups]
    fixed = [torch.randn(p.shape, generator=gen) * 0.1 for p in plist]
    max_norm = GC.CLIP_FRACTION * GC.global_norm(fixed)
    init = [p.detach().clone() for p in plist]
    results = {}
    for bound in (max_norm, 0.0):
        with torch.no_grad():
            for p, t in zip(plist, init):
                p.copy_(t)
        opt = AdamW([dict(g) for g in reference_param_groups(m, 3e-3)], lr=3e-3, max_grad_norm=bound, track_grad_norm=True)
        norms = []
        for scale in GC.STEP_SCALES:
            for p, x in zip(plist, fixed):
                p.grad = (x * scale).to(DEV)
            opt.step()
            norms.append(float(opt.last_grad_norm))
        results[bound] = ([p.detach().cpu().clone() for p in plist], norms)
        assert int(opt.skipped_steps) == 0
    got, norms = results[max_norm]
    assert norms[0] > max_norm and norms[1] > max_norm and norms[2] < max_norm, (norms, max_norm)
    rp = [t.cpu().double() for t in init]
    sizes = [len(g["params"]) for g in groups]
    rgroups, o = [], 0
    for g, k in zip(groups, sizes):
        rgroups.append(dict(params=rp[o:o + k], lr=g["lr"], weight_decay=g["weight_decay"]))
        o += k
    ref = GC.ClipAdamW64(rgroups, max_norm)
    for scale, n in zip(GC.STEP_SCALES, norms):
        rn, _ = ref.step([x * scale for x in fixed])
        assert abs(n - rn) <= 2.0 ** -23 * rn
    worst = 0.0
    for p, q in zip(got, rp):
        worst = max(worst, float(((p.double() - q).abs() / (1e-7 + 1e-6 * q.abs())).max()))
    print(f"worst error against the float64 restatement, in units of the bound: {worst:.3f}")
    for i, (p, q) in enumerate(zip(got, rp)):
        torch.testing.assert_close(p.double(), q, rtol=1e-6, atol=1e-7, msg=str(i))
    # without the bound the run must end somewhere else, or the comparison above proves nothing
    unclipped, _ = results[0.0]
    far = max(float(((p - q).abs() / (1e-7 + 1e-6 * q.abs())).max()) for p, q in zip(unclipped, got))
    assert far > 100.0, far


def _named_for_compare(model):
    # as test_build_optimizer_with_gradient_accumulation_equals_torch_adamw: the key bias has a pure-noise gradient whose sign Adam
    # amplifies to a full step, the word table's gradient is a float-atomic scatter-add (order-dependent last bits)
    return [(n, p) for n, p in model.named_parameters() if "key.bias" not in n and "word_embeddings" not in n]


def test_encoder_path_equals_torch_clip_grad_norm_in_front_of_the_unclipped_optimizer():
    from mtvaf_amd.optim import AdamW
    m, cfg = _model()
    m.eval()
    m2 = copy.deepcopy(m)  # (before the first forward pass: the layers' cached launch structures hold device pointers)
    batch = _batch(cfg)
    m(**batch).loss.backward()
    n0 = float(torch.nn.utils.clip_grad_norm_(m.parameters(), 1e30))  # (measures; a coefficient of 1 changes nothing)
    m.zero_grad(set_to_none=True)
    c = 0.5 * n0
    a = AdamW(m.parameters(), lr=1e-3, model=m, overlap=False, max_grad_norm=c)
    b = AdamW(m2.parameters(), lr=1e-3, model=m2, overlap=False)
    for it in range(2):
        m(**batch).loss.backward()
        a.step()
        ours = float(a.last_grad_norm)
        a.zero_grad(set_to_none=True)
        m2(**batch).loss.backward()
        theirs = float(torch.nn.utils.clip_grad_norm_(m2.parameters(), c))
        b.step()
        b.zero_grad(set_to_none=True)
        print(f"step {it}: norm {ours!r} torch {theirs!r} bound {c!r}")
        assert abs(ours - theirs) <= 1e-5 * theirs
        if it == 0:
            assert theirs > c  # the first step clips
    torch.cuda.synchronize()
    assert ("layer", 0) in a._flat_state and ("layer", 1) in a._flat_state  # one launch per layer was the path taken
    assert int(a.skipped_steps) == 0
    for (n, p), (_, q) in zip(_named_for_compare(m), _named_for_compare(m2)):
        atol = 2.5e-4 if (n.startswith("crf") or n.startswith("fc")) else 5e-6
        torch.testing.assert_close(p, q, rtol=0, atol=atol, msg=n)


def test_build_optimizer_with_a_bound_steps_after_the_backward_pass():
    import types
    from mtvaf_amd.optim import AdamW, build_optimizer
    m, _ = _model()
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, max_grad_norm=1.0)
    opt, _ = build_optimizer(m, args, 100)
    assert isinstance(opt, AdamW) and opt.overlap is False and opt.max_grad_norm == 1.0 and m.bert.encoder.grad_sink.on_layer_done is None
    m2, _ = _model()
    opt2, _ = build_optimizer(m2, types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, track_grad_norm=True), 100)
    assert opt2.overlap is False and opt2.track_grad_norm and opt2.max_grad_norm == 0.0


def _snapshot(model, opt):
    from mtvaf_amd import engine
    snap = {"p." + n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in model.named_parameters():
        st = opt.state.get(p, {})
        if "exp_avg" in st:
            snap["m." + n], snap["v." + n] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    for li, store in enumerate(model.bert.encoder._stores):
        w = store.weights
        if w._pl is not None:
            for k, img in enumerate(w._pl[2]):
                snap[f"planes.{li}.{k}"] = img.clone()
        sh = engine.shadow_for_update(w)
        if sh is not None:
            snap[f"shadow.{li}"] = sh.clone()
    return snap


def _same_bits(a, b):
    # (NaN-safe: compare the words)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step_and_leaves_every_copy_of_the_weights(bad, mode):
    from mtvaf_amd import hip
    from mtvaf_amd.optim import AdamW
    was = hip.COMPUTE
    hip.set_compute_dtype(mode)
    try:
        m, cfg = _model()
        m.eval()
        batch = _batch(cfg)
        opt = AdamW(m.parameters(), lr=1e-3, model=m, overlap=False, max_grad_norm=1.0)
        m(**batch).loss.backward()
        opt.step()  # a finite step first: moments, and the weight images the update maintains, exist
        opt.zero_grad(set_to_none=True)
        m(**batch).loss.backward()
        m.bert.encoder.layer[1].intermediate.dense.weight.grad[3, 5] = bad  # (a view into the layer's flat gradient buffer)
        before = _snapshot(m, opt)
        kinds = {k.split(".")[0] for k in before}
        assert {"p", "m", "v"} <= kinds and ("planes" in kinds if mode == "fp32" else "shadow" in kinds), kinds
        opt.step()
        after = _snapshot(m, opt)
        assert before.keys() == after.keys()
        for k in before:
            assert _same_bits(before[k], after[k]), k
        assert int(opt.skipped_steps) == 1 and not math.isfinite(float(opt.last_grad_norm))
        # the next finite step updates as usual
        opt.zero_grad(set_to_none=True)
        m(**batch).loss.backward()
        opt.step()
        later = _snapshot(m, opt)
        assert int(opt.skipped_steps) == 1 and math.isfinite(float(opt.last_grad_norm))
        w = "p.bert.encoder.layer.1.intermediate.dense.weight"
        assert not torch.equal(later[w], before[w]) and not torch.equal(later["p.fc.weight"], before["p.fc.weight"])
        assert all(bool(torch.isfinite(v).all()) for k, v in later.items() if k[0] in "pmv" and k[1] == ".")
        moved = [k for k in before if k.split(".")[0] in ("planes", "shadow") and not _same_bits(before[k], later[k])]
        assert moved  # the images followed the weights
    finally:
        hip.set_compute_dtype(was)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_without_the_skip_a_nonfinite_gradient_reaches_the_parameters_as_in_torch(bad):
    """torch.nn.utils.clip_grad_norm_ with an inf norm scales by 0 (inf * 0 = NaN in that element only), with a NaN norm by NaN
    (everything): the same here."""
    from mtvaf_amd.optim import AdamW
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(40, device=DEV)), torch.nn.Parameter(torch.randn(3, 5, device=DEV))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = AdamW(ps, lr=1e-2, max_grad_norm=1.0, skip_nonfinite=False)
    topt = torch.optim.AdamW(ref, lr=1e-2)
    for p, q in zip(ps, ref):
        p.grad = torch.randn_like(p)
        p.grad.view(-1)[2] = bad if p is ps[0] else 1.0
        q.grad = p.grad.clone()
    opt.step()
    torch.nn.utils.clip_grad_norm_(ref, 1.0)
    topt.step()
    assert int(opt.skipped_steps) == 0
    for p, q in zip(ps, ref):
        assert torch.equal(torch.isnan(p), torch.isnan(q))
    assert bool(torch.isnan(ps[0][2])) and (math.isinf(bad) or bool(torch.isnan(ps[1]).all()))


def test_defaults_issue_the_launches_of_the_unclipped_optimizer_and_allocate_nothing():
    """max_grad_norm = 0, track_grad_norm = False: no state, no workspace, the host-scalar entry points.  With a bound: state and
    workspace are allocated by the first step and reused by the next."""
    from mtvaf_amd import hip
    from mtvaf_amd.optim import AdamW
    ps = [torch.nn.Parameter(torch.randn(300, device=DEV)) for _ in range(3)]
    calls = []
    real = (hip.grad_sqnorm, hip.grad_clip_finalize, hip.adamw_multi)
    try:
        hip.grad_sqnorm = lambda *a, **k: (calls.append("sqnorm"), real[0](*a, **k))[1]
        hip.grad_clip_finalize = lambda *a, **k: (calls.append("finalize"), real[1](*a, **k))[1]
        hip.adamw_multi = lambda *a, **k: (calls.append("multi_dev" if k.get("clip") is not None else "multi"), real[2](*a, **k))[1]
        opt = AdamW(ps, lr=1e-3)
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
        assert calls == ["multi"] and opt.last_grad_norm is None and opt._clip_state is None
        del calls[:]
        opt = AdamW(ps, lr=1e-3, max_grad_norm=1.0)
        opt.step()
        ptrs = (opt._clip_state.data_ptr(), opt._clip_partials.data_ptr(), opt.skipped_steps.data_ptr(), opt.last_grad_norm.data_ptr())
        opt.step()
        assert calls == ["sqnorm", "finalize", "multi_dev"] * 2
        assert ptrs == (opt._clip_state.data_ptr(), opt._clip_partials.data_ptr(), opt.skipped_steps.data_ptr(),
                        opt.last_grad_norm.data_ptr())
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda and opt.skipped_steps.dtype == torch.int32
    finally:
        hip.grad_sqnorm, hip.grad_clip_finalize, hip.adamw_multi = real
