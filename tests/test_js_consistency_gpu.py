"""Cutoff consistency step of the span model on the MI355X: the mtvaf_js_consistency kernels against the float64 restatement
of the reference's cal_cut_loss / js_div (js_cases.py), and TVNetSAModel.forward_with_cutoff against the hand composition of
two forward calls and the consistency node."""
import functools

import pytest
import torch

import js_cases as J
import params as P
from test_model_gpu import DEV, LABELS, _prompt_inputs, close, hf_config, make_args

pytestmark = pytest.mark.gpu


def loss_close(got, ref):
    """the bound of the small loss kernels (test_span_gpu.py)"""
    got, ref = float(got), float(ref)
    print(f"loss got {got:.9e} ref {ref:.9e} err {abs(got - ref):.3e} allowed {1e-5 * abs(ref) + 1e-6:.3e}")
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-6, (got, ref)


@functools.lru_cache(maxsize=None)
def _reference(case):
    x, y = J.make_logits(*case)
    return (x, y) + J.ref_with_grads(x, y)


def _run(x, y, mask=None, scale=1.0, upstream=J.UPSTREAM):
    from mtvaf_amd import engine
    xg, yg = (t.clone().to(DEV).requires_grad_(True) for t in (x, y))
    js = engine.JSConsistencyFunction.apply(xg, yg, None if mask is None else mask.to(DEV), scale)
    assert js.dim() == 0 and js.dtype == torch.float32
    (js * upstream).backward()
    return js.detach(), xg.grad, yg.grad


@pytest.mark.parametrize("case", J.CASES, ids=J.case_id)
def test_kernel_matches_float64_restatement(case):
    x, y, ref, gx, gy = _reference(case)
    js, dx, dy = _run(x, y)
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all()
    loss_close(js, ref)
    close(dx, gx, rtol=1e-4, name="dlogits")
    close(dy, gy, rtol=1e-4, name="dcutoff_logits")


@pytest.mark.parametrize("idx", [0, 1], ids=[c[0] for c in J.masked_cases()])
def test_masked_kernel(idx):
    _, x, y, mask = J.masked_cases()[idx]
    ref, gx, gy = J.ref_with_grads(x, y, mask)
    js, dx, dy = _run(x, y, mask)
    assert torch.isfinite(js) and torch.isfinite(dx).all() and torch.isfinite(dy).all()
    loss_close(js, ref)
    close(dx, gx, rtol=1e-4, name="dlogits")
    close(dy, gy, rtol=1e-4, name="dcutoff_logits")
    dead = (mask == 0)[:, :, None].expand_as(x)
    assert not bool(dx.cpu()[dead].any()) and not bool(dy.cpu()[dead].any())      # exact zeros
    for b in range(x.shape[0]):
        if not bool(mask[b].any()):
            assert not bool(dx[b].any()) and not bool(dy[b].any())
    # a uint8 / bool mask is the same mask
    js8, dx8, _ = _run(x, y, mask.bool())
    assert torch.equal(js8, js) and torch.equal(dx8, dx)


def test_argument_forms():
    from mtvaf_amd import engine
    x, y, ref, gx, gy = _reference((5, 33, 4, 3, 1))
    js, dx, dy = _run(x, y)
    # a transposed view gives the bits of its contiguous copy
    xt = x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    yg = y.to(DEV).requires_grad_(True)
    assert not xt.is_contiguous()
    jt = engine.JSConsistencyFunction.apply(xt, yg)
    (jt * J.UPSTREAM).backward()
    assert torch.equal(jt.detach(), js) and torch.equal(xt.grad, dx) and torch.equal(yg.grad, dy)
    # the same tensor twice: two gradients, summed by autograd; the value is 0 within the loss bound
    xs = x.to(DEV).requires_grad_(True)
    same = engine.JSConsistencyFunction.apply(xs, xs)
    loss_close(same.detach(), 0.0)
    assert sum(fn is not None for fn, _ in same.grad_fn.next_functions) == 2
    same.backward()
    assert xs.grad is not None and xs.grad.shape == xs.shape and torch.isfinite(xs.grad).all()
    # scale rides in the kernel
    jq, dxq, dyq = _run(x, y, scale=0.25)
    loss_close(jq, 0.25 * ref)
    close(dxq, 0.25 * gx, rtol=1e-4, name="dlogits scale 0.25")
    close(dyq, 0.25 * gy, rtol=1e-4, name="dcutoff_logits scale 0.25")
    # other float dtypes are computed in fp32 and get gradients of their own dtype
    xd = x.double().to(DEV).requires_grad_(True)
    jd = engine.JSConsistencyFunction.apply(xd, y.to(DEV))
    jd.backward()
    assert torch.equal(jd, js) and xd.grad.dtype == torch.float64
    # the shape limits come back through hip._ck
    for shape in ((2, 20, 17), (2, 1025, 4)):
        z = torch.zeros(shape, device=DEV)
        with pytest.raises(RuntimeError, match="bad shape"):
            engine.JSConsistencyFunction.apply(z, z)
    with pytest.raises(ValueError):
        engine.JSConsistencyFunction.apply(torch.zeros(2, 20, 4, device=DEV), torch.zeros(2, 19, 4, device=DEV))


def test_forward_and_backward_are_deterministic():
    x, y = _reference((32, 20, 4, 3, 1))[:2]
    a, b = _run(x, y), _run(x, y)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- the model surface ------------------------------------------------------------------------------------------------
CFG = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
B, S, M = 6, 32, 5


def _build(use_prefix, dropout=0.0):
    from mtvaf_amd.models.bert_model import TVNetSAModel
    args = make_args(use_prefix=use_prefix, gcn_layer_number=0, num_layers=0, aug_type="span_cutoff", aug_cutoff_ratio=0.3)
    args.bert_config = hf_config(CFG, dropout=dropout)
    torch.manual_seed(0)
    return TVNetSAModel(LABELS, None, args).to(DEV), args


def _batch(use_prefix, B=B):
    lengths = [S, 20, 9, 31, 14, 26, 17, S][:B]
    ids, mask, tt, _ = P.text_batch(CFG, 3, B, S, lengths, lo_id=5)
    starts, ends, spos, epos, pol, lm = P.span_batch(CFG, 4, B, S, M, lengths)
    batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, start_positions=spos, end_positions=epos,
                 span_starts=starts, span_ends=ends, polarity_labels=pol, label_masks=lm)
    if use_prefix:
        feats, aux, _ = _prompt_inputs(11, B, 2)
        batch.update(images=feats, aux_imgs=aux)
    return {k: v.to(DEV) for k, v in batch.items()}


@pytest.fixture
def fixed_cut(monkeypatch):
    """Cutoff.span_keep with its uniform draw fixed, so that two cut passes cut the same rows"""
    from mtvaf_amd.modules.augument import Cutoff
    orig = Cutoff.span_keep
    u = torch.rand(8, generator=torch.Generator().manual_seed(5))
    monkeypatch.setattr(Cutoff, "span_keep", staticmethod(
        lambda lens, ratio, n_pos, u_=None: orig(lens, ratio, n_pos, u=u[:lens.shape[0]].to(lens.device))))


def _grads(m):
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


def _hand_composition(m, batch, a, b):
    from mtvaf_amd import engine
    plain, cut = m(**batch), m(**batch, augument=True)
    total = plain.loss + a * cut.loss + b * engine.JSConsistencyFunction.apply(plain.logits, cut.logits)
    total.backward()
    return total.detach(), _grads(m)


def test_model_with_nothing_cut_reduces_to_the_plain_loss():
    m, args = _build(False)
    m.eval()
    batch = _batch(False)
    args.aug_cutoff_ratio, args.aug_ce_loss, args.aug_js_loss = 0.0, 0.7, 1.0
    plain = m(**batch)
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    assert torch.equal(out.logits, plain.logits) and torch.equal(parts["cutoff_logits"], plain.logits)
    assert abs(float(parts["js"])) <= 1e-6
    want = (1 + 0.7) * float(plain.loss)
    assert abs(float(out.loss) - want) <= 1e-6 * abs(want)
    # without return_parts: the output alone
    alone = m.forward_with_cutoff(**batch)
    assert torch.equal(alone.loss, out.loss) and torch.equal(alone.logits, out.logits)


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (0.5, 2.0)])
def test_model_combined_loss_and_gradients(a, b, fixed_cut):
    m, args = _build(False)
    m.eval()
    batch = _batch(False)
    args.aug_ce_loss, args.aug_js_loss = a, b
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    assert not torch.equal(parts["cutoff_logits"], out.logits)
    js_ref = float(J.js_ref(out.logits.detach().cpu(), parts["cutoff_logits"].detach().cpu()))
    loss_close(parts["js"], js_ref)
    want = float(parts["loss"]) + a * float(parts["cutoff_loss"]) + b * js_ref
    assert abs(float(out.loss) - want) <= 1e-5 * abs(want), (float(out.loss), want)
    out.loss.backward()
    got = _grads(m)
    total, ref = _hand_composition(m, batch, a, b)
    assert abs(float(out.loss) - float(total)) <= 1e-5 * abs(float(total))
    assert set(got) == set(ref) and "bert.embeddings.word_embeddings.weight" in got
    for n in ref:
        close(got[n], ref[n], rtol=1e-3, name=n)


def test_model_weights_switch_terms_off(fixed_cut):
    m, args = _build(False)
    m.eval()
    batch = _batch(False)
    plain = m(**batch)
    args.aug_ce_loss, args.aug_js_loss = 1.0, 0.0
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    assert parts["js"] is None and parts["cutoff_logits"] is not None
    want = float(parts["loss"]) + float(parts["cutoff_loss"])
    assert abs(float(out.loss) - want) <= 1e-6 * abs(want)
    args.aug_ce_loss, args.aug_js_loss = 0.0, -1.0
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    assert torch.equal(out.loss, plain.loss) and torch.equal(out.logits, plain.logits)
    assert parts["js"] is None and parts["cutoff_loss"] is None and parts["cutoff_logits"] is None


def test_model_masked_consistency_term(fixed_cut):
    m, args = _build(False)
    m.eval()
    batch = _batch(False)
    args.aug_ce_loss, args.aug_js_loss, args.aug_js_masked = 1.0, 2.0, True
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    lm = batch["label_masks"].cpu()
    assert bool((lm == 0).any())
    logits, cut = out.logits.detach().cpu(), parts["cutoff_logits"].detach().cpu()
    js_ref = float(J.js_ref_masked(logits, cut, lm))
    assert abs(js_ref - float(J.js_ref(logits, cut))) > 1e-3 * js_ref     # the mask matters on this batch
    loss_close(parts["js"], js_ref)
    want = float(parts["loss"]) + float(parts["cutoff_loss"]) + 2.0 * js_ref
    assert abs(float(out.loss) - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("nb", [B, 8], ids=["B6", "B8-prompt-on-second-stream"])
def test_model_with_prefix_computes_the_prompt_once(nb, fixed_cut):
    m, args = _build(True)
    m.eval()
    batch = _batch(True, nb)
    args.aug_ce_loss, args.aug_js_loss = 1.0, 1.0
    calls, inner = [], m.get_visual_prompt

    def counted(images, aux_imgs):
        calls.append(1)
        return inner(images, aux_imgs)

    m.get_visual_prompt = counted
    out = m.forward_with_cutoff(**batch)
    assert len(calls) == 1
    out.loss.backward()
    got = _grads(m)
    total, ref = _hand_composition(m, batch, 1.0, 1.0)
    assert len(calls) == 3        # the hand composition computes it in both of its forward calls
    assert abs(float(out.loss) - float(total)) <= 1e-5 * abs(float(total))
    for n in ("encoder_conv.2.bias", "projectors.1.weight"):
        assert float(ref[n].abs().max()) > 0
        close(got[n], ref[n], rtol=5e-3, name=n)


def test_model_train_mode_step():
    m, args = _build(False, dropout=0.1)
    m.train()
    batch = _batch(False)
    args.aug_ce_loss, args.aug_js_loss = 1.0, 1.0
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    out, parts = m.forward_with_cutoff(**batch, return_parts=True)
    assert float(parts["js"]) > 0        # independent dropout masks and the cut: the passes differ
    out.loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
    gw = m.bert.embeddings.word_embeddings.weight.grad
    assert gw is not None and float(gw.abs().sum()) > 0
    opt.step()
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
