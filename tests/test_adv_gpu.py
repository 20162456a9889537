"""Adversarial step on the MI355X: mtvaf_adv_perturb against the float64 restatement and the derived
bound of adv_cases.py, the embedding tap, and Adversary.step against the hand composition
grad(loss(emb)) + weight * grad(loss(emb + delta_ref)) on the tiny models of test_model_gpu (dropout 0, eval mode: the passes are
comparable)."""
import copy
import types

import pytest
import torch

import adv_cases as A
import params as P
from test_js_consistency_gpu import _batch as span_batch, _build as span_build
from test_model_gpu import LABELS, close, hf_config, make_args
from test_ops_gpu import DEV, hip  # noqa: F401  (fixture)
from test_optim_gpu import _batch as tagger_batch

pytestmark = pytest.mark.gpu
IDS = [c["id"] for c in A.CASES]


def _run(hip, g, mask, eps=A.EPS, step=A.STEP, norm="l2", scope="sentence", delta_in=None, x=None):
    d, out, stats = hip.adv_perturb(g.to(DEV), mask.to(DEV), eps, step, norm, scope, delta_in=None if delta_in is None else delta_in.to(DEV),
                                    x=None if x is None else x.to(DEV))
    torch.cuda.synchronize()
    return d, out, stats


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", A.NORMS)
@pytest.mark.parametrize("scope", A.SCOPES)
@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_kernel_matches_the_restatement_within_the_derived_bound(hip, case, norm, scope):
    for mode in A.DELTA_MODES:
        g, mask, din = A.make_inputs(case, mode)
        x = torch.randn(g.shape, generator=torch.Generator().manual_seed(7))
        ref = A.reference(g, mask, A.EPS, A.STEP, norm, scope, delta_in=din)
        d, out, stats = _run(hip, g, mask, norm=norm, scope=scope, delta_in=din, x=x)
        e_d = A.excess(d, ref["delta"], ref["tol"])
        e_s = A.excess(stats, ref["stats"], ref["stats_tol"])
        print(f"{case['id']} {norm} {scope} delta_in={mode}: excess delta {e_d:.3f} stats {e_s:.3f}")
        assert e_d <= 1.0 and e_s <= 1.0, (mode, e_d, e_s)
        dead = mask.eq(0)
        assert not bool(d.cpu()[dead].any()), "dead rows are exact zeros"
        assert torch.equal(out, x.to(DEV) + d), "out is x + delta_out bit for bit"
        d2, out2, stats2 = _run(hip, g, mask, norm=norm, scope=scope, delta_in=din, x=x)
        assert torch.equal(d, d2) and torch.equal(out, out2) and torch.equal(stats, stats2), "same inputs, same bits"


def test_dead_rows_ignore_what_gradient_and_delta_in_hold_there(hip):
    case = A.CASES[2]
    g, mask, din = A.make_inputs(case, "bites")
    d0, _, s0 = _run(hip, g, mask, delta_in=din)
    g2, din2 = g.clone(), din.clone()
    g2[mask.eq(0)] = float("nan")
    din2[mask.eq(0)] = float("inf")
    d1, _, s1 = _run(hip, g2, mask, delta_in=din2)
    assert torch.equal(d0, d1) and torch.equal(s0, s1)
    # the vector body needs 16-byte aligned rows: a view one float into a buffer takes the scalar path and gives the same values
    buf = torch.zeros(g.numel() + 1, device=DEV)
    buf[1:] = g.to(DEV).view(-1)
    d2, _, s2 = hip.adv_perturb(buf[1:].view(g.shape), mask.to(DEV), A.EPS, A.STEP, delta_in=din.to(DEV))
    ref = A.reference(g, mask, A.EPS, A.STEP, delta_in=din)
    assert A.excess(d2, ref["delta"], ref["tol"]) <= 1.0 and A.excess(s2, ref["stats"], ref["stats_tol"]) <= 1.0


@pytest.mark.parametrize("scope", A.SCOPES)
def test_fgm_is_bit_identical_under_power_of_two_scales_of_the_gradient(hip, scope):
    """g * 2^k, k in -60 .. 60: every rounding of the kernel commutes with the scale.  An fp32 sum of squares fails at -60: the
    squares of elements around 1e-21 are subnormal or 0."""
    g, mask, _ = A.make_inputs(A.CASES[4])
    base, _, st0 = _run(hip, g, mask, scope=scope)
    assert float(base.abs().max()) > 0
    for k in (-60, -30, 0, 30, 60):
        d, _, st = _run(hip, g * 2.0 ** k, mask, scope=scope)
        assert torch.equal(d, base), f"k = {k}"
        assert torch.equal(st[:, 1], st0[:, 1]) and torch.equal(st[:, 0], st0[:, 0] * 2.0 ** k), f"stats, k = {k}"


@pytest.mark.parametrize("norm", A.NORMS)
@pytest.mark.parametrize("scope", A.SCOPES)
def test_degenerate_units(hip, norm, scope):
    case = A.CASES[2]
    g, mask, din = A.make_inputs(case, "bites")
    mask[2, :4] = 1
    g[2] = 0.0                                              # a sentence whose gradient is zero
    g[1, 2, 5], g[1, 3, 7] = float("inf"), float("nan")     # a sentence holding an inf and a NaN
    for delta_in in (None, din):
        ref = A.reference(g, mask, A.EPS, A.STEP, norm, scope, delta_in=delta_in)
        d, _, stats = _run(hip, g, mask, norm=norm, scope=scope, delta_in=delta_in)
        assert bool(torch.isfinite(d).all())
        assert A.excess(d, ref["delta"], ref["tol"]) <= 1.0
        st = stats.cpu()
        assert float(st[2, 0]) == 0.0 and not bool(torch.isfinite(st[1, 0])), "the zero and the non-finite norm are reported"
        assert A.excess(st[[0, 2]], ref["stats"][[0, 2]], ref["stats_tol"][[0, 2]]) <= 1.0
        assert A.excess(st[:, 1], ref["stats"][:, 1], ref["stats_tol"][:, 1]) <= 1.0
        if delta_in is None:
            assert not bool(d[2].any()) and (scope == "token" or not bool(d[1].any()))
            assert not bool(d[1, 2:4].any())


def test_bad_arguments_stop_at_the_host(hip):
    g, mask = torch.zeros(1, 4, 8, device=DEV), torch.ones(1, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.adv_perturb(torch.zeros(1, 513, 8, device=DEV), torch.ones(1, 513, dtype=torch.uint8, device=DEV), 1.0)
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.adv_perturb(torch.zeros(1, 2, 1025, device=DEV), torch.ones(1, 2, dtype=torch.uint8, device=DEV), 1.0)
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.adv_perturb(g, mask, float("nan"))
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.adv_perturb(g, mask, 1.0, step=-1.0)
    with pytest.raises(ValueError):
        hip.adv_perturb(g, mask, 1.0, norm="l1")
    with pytest.raises(ValueError):
        hip.adv_perturb(g, mask[:, :3], 1.0)
    with pytest.raises(ValueError):
        hip.adv_perturb(g, mask, 1.0, out=torch.empty_like(g))
    # masks of other dtypes are taken as non-zero = live
    d0 = hip.adv_perturb(g + 1.0, mask, 1.0)[0]
    for m in (mask.bool(), mask.long(), mask.float()):
        assert torch.equal(hip.adv_perturb(g + 1.0, m, 1.0)[0], d0)


# ---- 2. the tap --------------------------------------------------------------------------------------------------------
CFG = P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64)


def _tagger(use_prefix):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(alpha=0.0, use_prefix=use_prefix)
    args.bert_config = hf_config(CFG, dropout=0.0)
    torch.manual_seed(11)
    return TVNetSAModel2(LABELS, None, args).to(DEV).eval()


def _grads(m):
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


def test_tap_changes_nothing_until_it_is_given_a_delta():
    from mtvaf_amd import engine
    m = _tagger(True)
    batch = tagger_batch(CFG, B=8, S=32)
    assert m.bert.embedding_tap is None
    base = m(**batch).loss
    base.backward()
    g0 = _grads(m)
    m.bert.embedding_tap = None
    again = m(**batch).loss
    again.backward()
    g1 = _grads(m)
    tap = engine.EmbeddingTap(capture=True)
    m.bert.embedding_tap = tap
    try:
        tapped = m(**batch).loss
        tapped.backward()
    finally:
        m.bert.embedding_tap = None
    g2 = _grads(m)
    assert torch.equal(base, again) and torch.equal(base, tapped)
    assert set(g0) == set(g1) == set(g2) and "bert.embeddings.word_embeddings.weight" in g0
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]), n
    assert tap.grad is not None and tuple(tap.grad.shape) == (8, 32, CFG.hidden)
    # the same gradient as retain_grad() gives on the same tensor through get_embedding_output -> get_bert_output
    bert = m.bert
    emb = bert.get_embedding_output(batch["input_ids"], batch["token_type_ids"])
    emb.retain_grad()
    seq, _ = bert.get_bert_output(emb, attention_mask=batch["attention_mask"])
    w = torch.randn(seq.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * batch["attention_mask"][..., None]
    (seq * w).sum().backward()
    want = emb.grad.clone()
    m.zero_grad(set_to_none=True)
    tap = engine.EmbeddingTap(capture=True)
    bert.embedding_tap = tap
    try:
        emb2 = bert.get_embedding_output(batch["input_ids"], batch["token_type_ids"])
        seq2, _ = bert.get_bert_output(emb2, attention_mask=batch["attention_mask"])
        (seq2 * w).sum().backward()
    finally:
        bert.embedding_tap = None
    m.zero_grad(set_to_none=True)
    assert torch.equal(seq, seq2) and torch.equal(tap.grad, want)
    # a delta of zeros is x + 0: the same loss
    tap = engine.EmbeddingTap(delta=torch.zeros(8, 32, CFG.hidden, device=DEV))
    bert.embedding_tap = tap
    try:
        assert torch.equal(m(**batch).loss, base)
    finally:
        bert.embedding_tap = None


# ---- 3. end to end -----------------------------------------------------------------------------------------------------
def _hand_composition(m, batch, adv):
    """grad(loss(emb)) + sum_k weight / steps * grad(loss(emb + delta_k)), the deltas from the float64 restatement of the gradient
    a forward hook on the embeddings module keeps -- nothing of the tap or the kernel is used."""
    state = {"delta": None, "seen": None}

    def hook(mod, inp, out):
        if state["delta"] is not None:
            out = out + state["delta"]
        out.retain_grad()
        state["seen"] = out
        return out

    h = m.bert.embeddings.register_forward_hook(hook)
    try:
        m.zero_grad(set_to_none=True)
        loss = m(**batch).loss
        loss.backward()
        mask = batch["attention_mask"].cpu()
        delta, adv_losses = None, []
        for k in range(1, adv.steps + 1):
            g = state["seen"].grad.detach().cpu()
            first = adv.eps if adv.steps == 1 else min(adv.step_size, adv.eps)
            delta = A.reference(g, mask, first if k == 1 else adv.eps, adv.step_size, adv.norm, adv.scope, delta_in=delta)["delta"].float()
            state["delta"] = delta.to(DEV)
            lk = m(**batch).loss
            (lk * (adv.weight / adv.steps)).backward()
            adv_losses.append(lk.detach())
    finally:
        h.remove()
    return loss.detach(), sum(adv_losses) / adv.steps, _grads(m)


def _models():
    return {"tagger-prefix": lambda: (_tagger(True), tagger_batch(CFG, B=8, S=32)),
            "tagger-plain": lambda: (_tagger(False), tagger_batch(CFG, B=8, S=32)),
            "span": lambda: (span_build(False)[0].eval(), span_batch(False))}


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("which", ["tagger-prefix", "tagger-plain", "span"])
def test_step_equals_the_hand_composition(which, steps):
    from mtvaf_amd.adversarial import Adversary
    m, batch = _models()[which]()
    adv = Adversary(m, eps=1.0, steps=steps, weight=0.5)
    loss_ref, adv_ref, ref = _hand_composition(m, batch, adv)
    res = adv.step(**batch)
    assert m.bert.embedding_tap is None
    got = _grads(m)
    assert abs(float(res["loss"]) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    assert abs(float(res["adv_loss"]) - float(adv_ref)) <= 1e-4 * abs(float(adv_ref)) and float(res["adv_loss"]) != float(res["loss"])
    B = batch["input_ids"].shape[0]
    assert tuple(res["grad_norm"].shape) == (B,) and tuple(res["delta_norm"].shape) == (B,) and int(res["nonfinite"]) == 0
    want_norm = adv.eps if steps == 1 else None
    if want_norm is not None:
        assert torch.allclose(res["delta_norm"].cpu(), torch.full((B,), want_norm), rtol=1e-6)
    assert set(got) == set(ref) and "bert.embeddings.word_embeddings.weight" in got
    for n in ref:
        close(got[n], ref[n], rtol=1e-3, name=n)


def test_step_clears_the_tap_when_a_pass_raises():
    from mtvaf_amd.adversarial import Adversary
    m = _tagger(False)
    batch = tagger_batch(CFG, B=4, S=16)
    adv = Adversary(m, eps=1.0)
    with pytest.raises(TypeError):
        adv.step(**batch, no_such_key=1)
    assert m.bert.embedding_tap is None
    with pytest.raises(ValueError, match="labels"):
        adv.step(**{k: v for k, v in batch.items() if k != "labels"})
    assert m.bert.embedding_tap is None
    m.zero_grad(set_to_none=True)
    adv.step(**batch)
    assert m.bert.embedding_tap is None


def test_fused_accumulation_equals_the_fallback_after_the_optimizer_step():
    """AdamW(accumulation_steps=2): the clean pass writes the flat gradient buffers, the perturbed pass adds into them; the
    parameters after optimizer.step() against a copy of the model trained on the fallback (autograd adds)."""
    from mtvaf_amd.adversarial import Adversary
    from mtvaf_amd.optim import AdamW, reference_param_groups
    m1 = _tagger(True)
    m2 = copy.deepcopy(m1)
    batch = tagger_batch(CFG, B=8, S=32)
    o1 = AdamW(reference_param_groups(m1, 1e-3), model=m1, overlap=False)
    o2 = AdamW(reference_param_groups(m2, 1e-3), model=m2, overlap=False, accumulation_steps=2)
    with pytest.raises(ValueError, match="accumulation_steps=2"):
        Adversary(m2, steps=2, optimizer=o2)
    a1, a2 = Adversary(m1, eps=1.0, optimizer=o1), Adversary(m2, eps=1.0, optimizer=o2)
    r1, r2 = a1.step(**batch), a2.step(**batch)
    s2 = m2.bert.encoder.grad_sink
    assert s2.fast and s2.accumulate, "the perturbed pass added into the flat buffers"
    assert torch.equal(r1["loss"], r2["loss"])
    g1 = {n: p.grad.clone() for n, p in m1.named_parameters() if p.grad is not None}
    g2 = {n: p.grad.clone() for n, p in m2.named_parameters() if p.grad is not None}
    assert set(g1) == set(g2)
    for n in g1:
        close(g2[n], g1[n], rtol=1e-3, name="grad " + n)
    o1.step()
    o2.step()
    torch.cuda.synchronize()
    p2 = dict(m2.named_parameters())
    for n, p in m1.named_parameters():
        if p.requires_grad:
            close(p2[n], p, rtol=1e-3, name=n)


def test_build_optimizer_builds_the_adversary_only_when_asked():
    from mtvaf_amd.optim import build_optimizer
    m = _tagger(True)
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True)
    opt, _ = build_optimizer(m, args, 10)
    assert not hasattr(opt, "adversary") and opt.overlap is True
    m = _tagger(True)
    args.adv_eps, args.adv_steps = 0.5, 2
    opt, _ = build_optimizer(m, args, 10)
    assert opt.overlap is False and opt.accumulation_steps == 1 and opt.adversary.passes == 3 and opt.adversary.eps == 0.5
    m = _tagger(True)
    args.fused_accumulation = True
    opt, _ = build_optimizer(m, args, 10)
    assert opt.overlap is True and opt.accumulation_steps == 3 and opt.adversary.optimizer is opt
    batch = tagger_batch(CFG, B=8, S=32)
    w0 = m.bert.encoder.layer[0].intermediate.dense.weight
    before = w0.detach().clone()
    res = opt.adversary.step(**batch)  # the last pass updates the layers from inside its backward
    torch.cuda.synchronize()
    assert not torch.equal(w0.detach(), before) and bool(torch.isfinite(res["adv_loss"]))
    opt.step()
    opt.zero_grad()
