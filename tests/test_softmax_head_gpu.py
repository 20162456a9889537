"""TVNetSAModel2 with the token cross entropy on the MI355X: args.token_ce_weight beside the CRF, and
args.tag_head = "softmax" -- loss, tags, `predict`, the entity scorer and what is refused -- against the float64 restatement of
token_ce_cases.py on the model's own emissions.  Small models: B 3, S 12, 2 layers, eval mode (no dropout)."""
import types

import pytest
import torch
from transformers import BertConfig

import entity_cases as E
import params as P
import token_ce_cases as T
from test_model_gpu import DEV, close
from test_token_ce_gpu import value_close

pytestmark = pytest.mark.gpu
LABELS = E.SET_A
LABEL_MAP = {label: i for i, label in enumerate(LABELS, 1)}
C = len(LABELS) + 1
B, S = 3, 12


def tiny_model(**kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=False, vao=False, noauxloss=True, use_probe=False,
                                 n_gpu=1, alpha=0.5, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV, resnet_root=None,
                                 use_152=False, **kw)
    args.bert_config = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                                  num_attention_heads=cfg.heads, intermediate_size=cfg.inter,
                                  max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.eps,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    m = TVNetSAModel2(LABELS, None, args).to(DEV).eval()
    with torch.no_grad():  # an untrained head decodes mostly one tag: spread the emissions
        m.fc.weight.mul_(40.0)
    return cfg, m


def batch(cfg, seed=40):
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, seed, B, S, lo_id=5))
    labels[:, 0] = LABEL_MAP["[CLS]"]
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt), mask, labels


def run(m, kw, labels):
    """One forward + backward with the hidden states the head read -> (output, hidden [B,S,H] detached, gradients by name)"""
    cap = {}
    hook = m.bert.register_forward_hook(lambda mod, inp, out: cap.update(h=out["last_hidden_state"]))
    m.zero_grad(set_to_none=True)
    out = m(labels=labels, **kw)
    hook.remove()
    out.loss.backward()
    return out, cap["h"].detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def restated(m, hidden, labels, mask, reduction="batch_mean", weight=None, smoothing=0.0, gamma=0.0):
    """The restatement on float64 emissions of the model's own hidden states -> (value, d value / d fc.weight, emissions)"""
    h = hidden.double().cpu().view(-1, hidden.shape[-1])
    W = m.fc.weight.detach().double().cpu().requires_grad_(True)
    em = h @ W.t() + m.fc.bias.detach().double().cpu()
    loss, _ = T.token_ce_ref(em, labels.cpu().view(-1), mask.cpu().view(-1).to(torch.uint8), weight, smoothing, gamma, reduction, B)
    (gW,) = torch.autograd.grad(loss, (W,))
    return loss.detach(), gW, em.detach().view(B, S, -1)


def test_auxiliary_term_beside_the_crf():
    cfg, plain = tiny_model()
    _, aux = tiny_model(token_ce_weight=0.5)
    assert plain.token_ce is None and aux.token_ce is not None and not list(aux.token_ce.parameters())
    assert set(aux.state_dict()) == set(plain.state_dict())
    aux.load_state_dict(plain.state_dict())
    kw, mask, labels = batch(cfg)
    a, hidden, ga = run(plain, kw, labels)
    b, hidden_b, gb = run(aux, kw, labels)
    assert torch.equal(hidden, hidden_b) and list(a.logits) == list(b.logits) and plain.last_token_ce is None
    ce, gW, _ = restated(aux, hidden, labels, mask)
    assert float(ce) > 0.1
    value_close(aux.last_token_ce, ce, "last_token_ce")
    value_close(b.loss, a.loss.detach().double().cpu() + 0.5 * ce, "loss")
    close(gb["fc.weight"], ga["fc.weight"].double().cpu() + 0.5 * gW, rtol=1e-4, name="fc.weight.grad")
    for n in ("crf.transitions", "crf.start_transitions", "crf.end_transitions"):
        assert torch.equal(ga[n], gb[n]), n   # the term does not reach the chain
    # without labels nothing is added and nothing is kept
    aux(**kw)
    assert aux.last_token_ce is None


@pytest.mark.parametrize("options", [dict(), dict(token_ce_reduction="mean", token_ce_smoothing=0.1, token_ce_focal_gamma=2.0,
                                                 token_ce_class_weights="structural")], ids=["default", "all"])
def test_softmax_head_loss_and_tags(options):
    from mtvaf_amd.metrics import label_sequences
    weight = None
    if options:
        weight = torch.ones(C)
        for name in ("X", "[CLS]", "[SEP]"):
            weight[LABEL_MAP[name]] = 0.0
        weight[0] = 0.0   # PAD
        options = dict(options, token_ce_class_weights=weight.tolist())
    cfg, m = tiny_model(tag_head="softmax", score_entities=True, **options)
    assert not any(n.startswith("crf.") for n in m.state_dict()) and not any(n.startswith("crf.") for n, _ in m.named_parameters())
    assert not bool(m.crf.transitions.any()) and m.crf.transitions.device.type == "cuda"
    kw, mask, labels = batch(cfg)
    out, hidden, grads = run(m, kw, labels)
    ref, gW, em = restated(m, hidden, labels, mask, options.get("token_ce_reduction", "batch_mean"), weight,
                           options.get("token_ce_smoothing", 0.0), options.get("token_ce_focal_gamma", 0.0))
    assert float(ref) > 0.1
    value_close(out.loss, ref)
    close(grads["fc.weight"], gW, rtol=1e-4, name="fc.weight.grad")
    # the tags are the kernel's first maxima, on the device for the scorer
    emissions = torch.nn.functional.linear(hidden, m.fc.weight, m.fc.bias)
    tags, logp = m.token_ce.decode(emissions, mask)
    lens = mask.sum(1).tolist()
    assert list(out.logits) == [tags[r, :lens[r]].tolist() for r in range(B)]
    dt = out.logits.device_tags
    assert dt.dtype == torch.int32 and dt.is_cuda and tuple(dt.shape) == (B, S)
    assert torch.equal(dt.long(), torch.where(mask != 0, tags, torch.full_like(tags, -1)))
    y_true, y_pred = label_sequences(labels, mask, out.logits, LABEL_MAP)
    as_labels = lambda rows: [[(n, n == "O") for n in row] for row in rows]  # noqa: E731
    sc = m.entity_scorer
    want = E.counter(sc.types, E.count_sequences("seqeval", as_labels(y_true), as_labels(y_pred)))
    assert sc.counts.cpu().numpy().tolist() == want.tolist() and want[-1] > 0

    # predict: the same tags; every entity's confidence is the sum of its tokens' log-probabilities
    res = m.predict(**kw)
    assert torch.equal(res["tags"].long(), dt.long())
    # (`CRF.entities` forms log p(segment) as the difference of two log-partition functions of the sentence: its error is that
    # cancellation's, so the bound is the one of tests/test_crf_entities_gpu.py, 2e-5 * max|logZ|, with logZ of the zero chain
    # = the sum of the live tokens' logsumexp, in float64)
    ents, lc = res["entities"].cpu().numpy(), res["log_confidence"].double().cpu()
    lp = logp.double().cpu()
    logz = (torch.logsumexp(em, -1) * (mask.cpu() != 0)).sum(1)
    bound = 2e-5 * float(logz.abs().max())
    n = 0
    for r in range(B):
        for e in range(ents.shape[1]):
            s, t, _ = ents[r, e]
            if s < 0:
                assert float(res["confidence"][r, e]) == 0.0
                continue
            want = float(lp[r, s:t + 1].sum())
            print(f"log_confidence[{r},{e}]: err {abs(float(lc[r, e]) - want):.3e}, bound {bound:.3e}")
            assert abs(float(lc[r, e]) - want) <= bound
            assert float(res["confidence"][r, e]) == float(torch.exp(res["log_confidence"][r, e]))
            n += 1
    assert n >= 2, "the batch holds too few entities to show anything"


def test_softmax_head_refuses_what_needs_a_chain():
    cfg, m = tiny_model(tag_head="softmax")
    kw, mask, labels = batch(cfg)
    from mtvaf_amd.constraints import sets_from_labels
    allowed = sets_from_labels(labels, C)
    for call in (lambda: m(allowed_tags=allowed, **kw), lambda: m.forward_consistent(allowed_tags=allowed, **kw),
                 lambda: m.predict_constrained(**kw), lambda: m.predict_posteriors(**kw), lambda: m.predict_nbest(**kw)):
        with pytest.raises(ValueError, match="tag_head"):
            call()
    for bad in (dict(crf_risk_weight=0.5), dict(crf_mrt_weight=0.5), dict(crf_entropy_weight=-0.1), dict(crf_reduction="sum"),
                dict(consistency_level="chain")):
        with pytest.raises(ValueError, match="tag_head"):
            tiny_model(tag_head="softmax", **bad)
    # the token-level consistency step works: two passes without dropout agree, so the divergence is 0 and the loss is the CE
    _, r = tiny_model(tag_head="softmax", consistency_weight=1.0)
    r.load_state_dict(m.state_dict())
    out, parts = r.forward_consistent(labels=labels, return_parts=True, **kw)
    plain = m(labels=labels, **kw)
    assert float(parts["divergence"]) == 0.0 and torch.equal(out.loss, plain.loss) and list(out.logits) == list(plain.logits)


def test_defaults_launch_what_they_launched():
    """No new option set: loss, tags and every gradient are the bits of a model whose args lack the attributes."""
    cfg, plain = tiny_model()
    _, named = tiny_model(tag_head="crf", token_ce_weight=0.0, token_ce_reduction="batch_mean", token_ce_smoothing=0.0,
                          token_ce_focal_gamma=0.0, token_ce_class_weights=None)
    named.load_state_dict(plain.state_dict())
    assert named.token_ce is None and set(named.state_dict()) == set(plain.state_dict())
    kw, mask, labels = batch(cfg)
    a, _, ga = run(plain, kw, labels)
    b, _, gb = run(named, kw, labels)
    assert torch.equal(a.loss, b.loss) and list(a.logits) == list(b.logits) and set(ga) == set(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
