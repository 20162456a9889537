"""The tagger's two-pass consistency step on the MI355X: CRF.symmetric_kl against the two kl_divergence calls it replaces, and
TVNetSAModel2.forward_consistent against the step assembled by hand from two encoder calls."""
import math

import pytest
import torch

import crf_path_cases as Pc
import params as P
import token_div_cases as T
from test_crf_path_gpu import _crf, _dev
from test_model_gpu import DEV, LABELS, _prompt_inputs, close, hf_config, make_args

pytestmark = pytest.mark.gpu

CFG = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
B, S, LENGTHS = 3, 16, [16, 9, 5]


# ---- CRF.symmetric_kl -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (3, 17, 17, 1)], ids=str)
def test_symmetric_kl_is_the_sum_of_the_two_kl_divergences(shape):
    """Value and every gradient, transitions included, against kl_divergence(a,b) + kl_divergence(b,a) in float64
    (crf_path_cases.kl_oracle, both directions).  The bound of each quantity is kl_divergence's for the a||b direction
    (crf_path_cases.kl_reference) plus, for b||a, the floor that bound never goes below (crf_path_cases.bound: 2e-5 max|logZ| for the
    value, 1e-4 max|ref| + 1e-7 for a gradient) -- no more than the sum of the two bounds test_crf_path_gpu.py applies."""
    fwd = Pc.kl_reference(shape, True)
    rev = Pc.kl_oracle(fwd.q, fwd.p, fwd.w, True)
    floor = lambda k: 2e-5 * float(rev["logz"].max()) if k == "kl" else 1e-4 * float(rev[k].abs().max()) + 1e-7
    pairs = {"kl": ("kl", "kl"), "dem_a": ("dem_p", "dem_q"), "dem_b": ("dem_q", "dem_p"), "dstart": ("dstart_p", "dstart_p"),
             "dend": ("dend_p", "dend_p"), "dtrans": ("dtrans_p", "dtrans_p")}
    ref = {k: fwd.r64[f] + rev[r] for k, (f, r) in pairs.items()}
    bnd = {k: fwd.bound[f] + floor(r) for k, (f, r) in pairs.items()}
    ea, _, mask, start, end, trans = _dev(*fwd.p)
    eb = fwd.q[0].to(DEV)
    crf = _crf(shape[2], start, end, trans)
    a, b = ea.clone().requires_grad_(True), eb.clone().requires_grad_(True)
    skl = crf.symmetric_kl(a, b, mask, reduction="none")
    assert skl.shape == (shape[0],)
    (skl * fwd.w.to(DEV)).sum().backward()
    got = {"kl": skl, "dem_a": a.grad, "dem_b": b.grad, "dstart": crf.start_transitions.grad, "dend": crf.end_transitions.grad,
           "dtrans": crf.transitions.grad}
    for k in ref:
        err = float((got[k].detach().double().cpu() - ref[k]).abs().max())
        print(f"symmetric_kl {k}: err {err:.3e} bound {bnd[k]:.3e}")
        assert err <= bnd[k], (k, err, bnd[k])
    # the reductions, and the sum of the module's own two calls
    live = float(Pc.live(fwd.p[2]).sum())
    with torch.no_grad():
        assert torch.equal(crf.symmetric_kl(ea, eb, mask), skl.detach().mean())
        assert torch.equal(crf.symmetric_kl(ea, eb, mask, reduction="sum"), skl.detach().sum())
        tm = crf.symmetric_kl(ea, eb, mask, reduction="token_mean")
        assert abs(float(tm) - float(skl.detach().sum()) / live) <= 1e-6 * abs(float(tm))
        two = crf.kl_divergence(ea, eb, mask) + crf.kl_divergence(eb, ea, mask)
        assert float((two - skl.detach()).abs().max()) <= 2 * bnd["kl"]
        # one tensor on both sides: exactly 0
        assert not bool(crf.symmetric_kl(ea, ea, mask, reduction="none").any())
    with pytest.raises(ValueError):
        crf.symmetric_kl(ea, eb[:, :-1], mask)
    with pytest.raises(ValueError):
        crf.symmetric_kl(ea, eb, mask, reduction="batch")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _build(use_prefix=False, dropout=0.0, **kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(use_prefix=use_prefix, aug_cutoff_ratio=0.3, **kw)
    args.bert_config = hf_config(CFG, dropout=dropout)
    torch.manual_seed(0)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    with torch.no_grad():  # an untrained head gives nearly flat emissions: spread them
        m.fc.weight.mul_(40.0)
    m.dropout.p = dropout
    return m, args


def _batch(use_prefix=False):
    ids, mask, tt, labels = P.text_batch(CFG, 3, B, S, LENGTHS, lo_id=5)
    batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
    if use_prefix:
        feats, aux, lab = _prompt_inputs(11, B, 2)
        batch.update(images=feats, aux_imgs=aux, imagelabel=lab)
    return {k: v.to(DEV) for k, v in batch.items()}


def _grads(m):
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


def _divergence_fp32(e1, e2, mask, kind, temperature=1.0):
    """The restatement's formula (token_div_cases.row_values, masked token mean) in fp32 torch ops, differentiable"""
    lp, lq = torch.log_softmax(e1 / temperature, -1), torch.log_softmax(e2 / temperature, -1)
    p, q = lp.exp(), lq.exp()
    if kind == "sym_kl":
        rows = 0.5 * ((p - q) * (lp - lq)).sum(-1)
    else:
        lm = torch.logaddexp(lp, lq) - math.log(2.0)
        rows = 0.5 * (p * (lp - lm)).sum(-1) + 0.5 * (q * (lq - lm)).sum(-1)
    live = mask != 0
    return (rows * live).sum() / live.sum()


def _by_hand(m, args, batch, level="token", kind="sym_kl", second_pass_trains=True):
    """The step from two encoder calls on one prompt: -> (loss, parts, gradients)"""
    from mtvaf_amd import engine
    mask = batch["attention_mask"]
    prefix, full = None, mask
    if args.use_prefix:
        prefix = m.get_visual_prompt(batch["images"], batch["aux_imgs"], batch["imagelabel"])[0]
        full = torch.cat([torch.ones(B, prefix[0][0].shape[2], dtype=mask.dtype, device=DEV), mask], 1)
    ems = []
    for _ in range(2):
        hidden = m.bert(input_ids=batch["input_ids"], attention_mask=full, token_type_ids=batch["token_type_ids"],
                        past_key_values=prefix, output_hidden_states=True, return_dict=True)["last_hidden_state"]
        ems.append(engine.LinearFunction.apply(engine.dropout(hidden, m.dropout.p, m.training), m.fc.weight, m.fc.bias, False))
    e1, e2 = ems[0], ems[1] if second_pass_trains else ems[1].detach()
    m8 = mask.to(torch.uint8)
    nll_1, nll_2 = m.crf.nll_mean(e1, batch["labels"], mask=m8), m.crf.nll_mean(e2, batch["labels"], mask=m8)
    if level == "token":
        div = _divergence_fp32(e1, e2, mask, kind, getattr(args, "consistency_temperature", 1.0))
    else:
        div = (m.crf.kl_divergence(e1, e2, m8) + m.crf.kl_divergence(e2, e1, m8)).sum() / (mask != 0).sum()
    loss = 0.5 * (nll_1 + nll_2) + args.consistency_weight * div
    loss.backward()
    return loss.detach(), dict(nll=nll_1.detach(), nll_2=nll_2.detach(), divergence=div.detach(), emissions=e1.detach(),
                               emissions_2=e2.detach()), _grads(m)


def test_eval_mode_without_a_cut_is_the_plain_step():
    m, args = _build()
    m.eval()
    batch = _batch()
    plain = m(**batch)
    args.consistency_weight = 1.5
    out, parts = m.forward_consistent(**batch, return_parts=True)
    assert torch.equal(parts["emissions_2"], parts["emissions"]) and float(parts["divergence"]) <= 1e-6
    assert abs(float(out.loss.detach()) - float(plain.loss.detach())) <= 1e-6 * abs(float(plain.loss.detach()))
    assert list(out.logits) == list(plain.logits)
    alone = m.forward_consistent(**batch)  # without return_parts: the output alone
    assert torch.equal(alone.loss, out.loss) and list(alone.logits) == list(out.logits)
    # the defaults: no divergence; with consistency_ce off as well no second pass -- forward's loss, bit for bit
    args.consistency_weight, args.consistency_ce = 0.0, False
    out, parts = m.forward_consistent(**batch, return_parts=True)
    assert torch.equal(out.loss, plain.loss) and parts["emissions_2"] is None and parts["nll_2"] is None and parts["divergence"] is None
    with pytest.raises(ValueError, match="labels or allowed_tags"):
        m.forward_consistent(**{k: v for k, v in batch.items() if k != "labels"})


@pytest.mark.parametrize("level,kind", [("token", "sym_kl"), ("token", "js"), ("chain", "sym_kl")])
def test_train_mode_step_matches_the_hand_assembly(level, kind):
    from mtvaf_amd import engine
    m, args = _build(use_prefix=True, dropout=0.1)
    m.train()
    batch = _batch(True)
    args.consistency_weight, args.consistency_level, args.consistency_kind, args.consistency_temperature = 0.7, level, kind, 2.0
    engine.RNG.offset = 1000
    out, parts = m.forward_consistent(**batch, return_parts=True)
    assert not torch.equal(parts["emissions_2"], parts["emissions"]) and float(parts["divergence"]) > 0
    want = 0.5 * (float(parts["nll"]) + float(parts["nll_2"])) + 0.7 * float(parts["divergence"])
    assert abs(float(out.loss.detach()) - want) <= 1e-5 * abs(want)
    out.loss.backward()
    got = _grads(m)
    engine.RNG.offset = 1000
    loss, hand, ref = _by_hand(m, args, batch, level, kind)
    assert torch.equal(hand["emissions"], parts["emissions"].detach()) and torch.equal(hand["emissions_2"], parts["emissions_2"].detach())
    if level == "token":
        ref64 = T.token_div_ref(hand["emissions"].cpu().view(B * S, -1), hand["emissions_2"].cpu().view(B * S, -1),
                                batch["attention_mask"].cpu().view(-1), kind, 2.0)[0]
        assert abs(float(parts["divergence"]) - float(ref64)) <= 1e-5 * abs(float(ref64)) + 1e-6
    assert abs(float(parts["divergence"]) - float(hand["divergence"])) <= 1e-4 * abs(float(hand["divergence"]))
    assert abs(float(out.loss.detach()) - float(loss)) <= 1e-5 * abs(float(loss))
    assert set(got) == set(ref)
    for n in ref:
        close(got[n], ref[n], rtol=1e-3, name=n)
    # both passes train: with pass 2 detached the shared parameters get another gradient
    engine.RNG.offset = 1000
    _, _, one = _by_hand(m, args, batch, level, kind, second_pass_trains=False)
    for n in ("bert.embeddings.word_embeddings.weight", "encoder_conv.2.weight"):
        assert float(got[n].abs().max()) > 0
        assert float((got[n] - one[n]).abs().max()) > 1e-2 * float(got[n].abs().max()), n


def test_fused_accumulation_shares_the_flat_buffers():
    m, args = _build()
    m.eval()
    batch = _batch()
    args.consistency_weight, args.consistency_aug = 1.0, "dim_cutoff"
    torch.manual_seed(7)
    m.forward_consistent(**batch).loss.backward()
    ref = {n: p.grad.clone() for n, p in m.bert.encoder.named_parameters()}
    m.zero_grad(set_to_none=True)
    sink = m.bert.encoder.grad_sink
    setting = (sink.accumulate_passes, sink.nodes_per_pass)
    args.fused_accumulation = True
    torch.manual_seed(7)
    out = m.forward_consistent(**batch)
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (1, 2)
    out.loss.backward()
    torch.cuda.synchronize()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == setting, "back to its setting when the pass ended"
    for n, p in m.bert.encoder.named_parameters():  # (the bound of test_accumulation_gpu.py's cutoff step: the same bits)
        assert torch.equal(p.grad, ref[n]), n
    m.zero_grad(set_to_none=True)
    # an exception inside the passes: the sink is back as well
    def fails(*a, **kw):
        assert (sink.accumulate_passes, sink.nodes_per_pass) == (1, 2)
        raise RuntimeError("inside the passes")

    m._crf_nll = fails
    with pytest.raises(RuntimeError, match="inside the passes"):
        m.forward_consistent(**batch)
    assert (sink.accumulate_passes, sink.nodes_per_pass) == setting and sink._two_node_saved is None


@pytest.mark.parametrize("aug", ["span_cutoff", "token_cutoff", "dim_cutoff"])
def test_every_cut_runs_under_the_uncut_crf_mask(aug):
    m, args = _build(use_prefix=True)
    m.eval()
    batch = _batch(True)
    args.consistency_weight, args.consistency_aug = 1.0, aug
    torch.manual_seed(3)
    out, parts = m.forward_consistent(**batch, return_parts=True)
    assert not torch.equal(parts["emissions_2"], parts["emissions"])
    assert all(bool(torch.isfinite(parts[k]).all()) for k in ("nll", "nll_2", "divergence")) and bool(torch.isfinite(out.loss))
    assert [len(p) for p in out.logits] == LENGTHS
    m8 = batch["attention_mask"].to(torch.uint8)
    assert torch.equal(parts["nll_2"], m.crf.nll_mean(parts["emissions_2"], batch["labels"], mask=m8))  # the whole prefix mask
    out.loss.backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


def test_word_pooling_runs_the_divergence_on_the_word_axis():
    m, args = _build(dropout=0.1, word_pooling="first", max_words=10)
    m.train()
    batch = _batch()
    pos = torch.arange(S, device=DEV, dtype=torch.int32).expand(B, -1)
    t2w = torch.where(batch["attention_mask"] != 0, pos // 2, torch.full_like(pos, -1))
    args.consistency_weight = 1.0
    out, parts = m.forward_consistent(**batch, token_to_word=t2w, return_parts=True)
    assert parts["emissions"].shape == parts["emissions_2"].shape == (B, 10, len(LABELS) + 1)
    assert [len(p) for p in out.logits] == [(n + 1) // 2 for n in LENGTHS]
    wm = m.last_word_index.word_mask
    ref = T.token_div_ref(parts["emissions"].detach().cpu().view(B * 10, -1), parts["emissions_2"].detach().cpu().view(B * 10, -1),
                          wm.cpu().view(-1), "sym_kl")[0]
    assert float(ref) > 0 and abs(float(parts["divergence"]) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-6
    out.loss.backward()
    assert float(m.bert.embeddings.word_embeddings.weight.grad.abs().max()) > 0


def test_layer_mix_serves_both_passes():
    m, args = _build(dropout=0.1, layer_mix="all")
    m.train()
    args.consistency_weight = 1.0
    out, parts = m.forward_consistent(**_batch(), return_parts=True)
    assert float(parts["divergence"]) > 0
    out.loss.backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m.layer_mix.parameters())


def test_vao_loss_enters_once():
    m, args = _build(use_prefix=True, vao=True)
    m.eval()
    batch = _batch(True)
    args.consistency_weight = 1.0
    calls, inner = [], m.get_visual_prompt

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)

    m.get_visual_prompt = counted
    out, parts = m.forward_consistent(**batch, return_parts=True)
    assert len(calls) == 1
    img = float(inner(batch["images"], batch["aux_imgs"], batch["imagelabel"])[1])
    assert img > 0
    want = 0.5 * (float(parts["nll"]) + float(parts["nll_2"])) + float(parts["divergence"]) + args.alpha * img
    assert abs(float(out.loss.detach()) - want) <= 1e-5 * abs(want)
    assert abs(float(out.loss.detach()) - float(m(**batch).loss.detach())) <= 1e-5 * abs(want)  # eval mode, no cut: forward's loss, alpha * img once


def test_forward_is_untouched_by_a_consistent_step():
    from mtvaf_amd import engine
    m, args = _build(use_prefix=True, dropout=0.1)
    m.train()
    batch = _batch(True)
    args.consistency_weight, args.consistency_aug = 1.0, "span_cutoff"
    engine.RNG.offset = 1000
    before = m(**batch)
    m.forward_consistent(**batch).loss.backward()
    m.zero_grad(set_to_none=True)
    engine.RNG.offset = 1000
    after = m(**batch)
    assert torch.equal(after.loss, before.loss) and list(after.logits) == list(before.logits)
