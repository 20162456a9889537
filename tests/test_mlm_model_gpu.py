"""TVNetSAModel2 with the masked-LM head on the MI355X: `forward_mlm` under the image prefix, the
auxiliary term of `forward` (args.mlm_weight), and the head's place in `optim.build_optimizer`.  Tiny dimensions: B 3, S 16, P 4
(one image, no crops), 2 layers."""
import types

import pytest
import torch
from transformers import BertConfig

import params as P
from test_model_gpu import DEV

pytestmark = pytest.mark.gpu
LABELS = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]
B, S = 3, 16
CFG = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
MLM = dict(mlm_mask_token_id=4, mlm_special_ids=(0, 1, 2, 3, 4))


def tiny_model(dropout=0.0, **kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=True, vao=False, noauxloss=True, use_probe=False, n_gpu=1,
                                 alpha=0.0, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV, resnet_root=None, use_152=False,
                                 lr=1e-3, warmup_ratio=0.0, **kw)
    args.bert_config = BertConfig(vocab_size=CFG.vocab_size, hidden_size=CFG.hidden, num_hidden_layers=CFG.layers,
                                  num_attention_heads=CFG.heads, intermediate_size=CFG.inter, max_position_embeddings=CFG.max_pos,
                                  type_vocab_size=CFG.type_vocab, layer_norm_eps=CFG.eps, hidden_dropout_prob=dropout,
                                  attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    return TVNetSAModel2(LABELS, None, args).to(DEV), args


def batch():
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(CFG, 61, B, S, lengths=[16, 9, 5], lo_id=5))
    labels[:, 0] = 9
    g = torch.Generator().manual_seed(62)
    return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, images=torch.rand(B, 3840, 2, 2, generator=g).to(DEV),
                aux_imgs=None), labels


def step(m, labels=None, seed=7, **kw):
    """One forward + backward at a fixed dropout / masking state -> (loss, gradients by name)"""
    from mtvaf_amd import engine
    torch.manual_seed(seed)
    engine.RNG.offset = 500
    m.zero_grad(set_to_none=True)
    out = None if labels is not None else m.forward_mlm(**kw)
    if labels is not None:
        out = m(labels=labels, **kw)
        step.paths = list(out.logits)
        out = out.loss
    out.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_forward_mlm_trains_head_table_encoder_and_prompt_generator():
    m, _ = tiny_model(mlm_head=True, **MLM)
    m.train()
    kw, _ = batch()
    loss, g = step(m, **kw, mlm_probability=0.5)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    assert int(m.mlm_head.last_count) > 0 and m.last_mlm_stats.tolist()[2] == 0 and 0.0 <= float(m.mlm_head.last_accuracy) <= 1.0
    reached = ["mlm_head.predictions.bias", "mlm_head.predictions.transform.dense.weight", "mlm_head.predictions.transform.LayerNorm.weight",
               "bert.embeddings.word_embeddings.weight", "bert.encoder.layer.0.attention.self.query.weight",
               "bert.encoder.layer.1.output.dense.weight", "encoder_conv.0.weight", "encoder_conv.2.bias", "projectors.0.weight"]
    for n in reached:
        assert n in g and bool(torch.isfinite(g[n]).all()) and float(g[n].abs().max()) > 0, n
    assert "fc.weight" not in g and "crf.transitions" not in g  # the tagging head takes no part
    again, g2 = step(m, **kw, mlm_probability=0.5)  # the same generator state: the same bits
    assert torch.equal(loss, again) and all(torch.equal(g[n], g2[n]) for n in reached)


def test_weight_zero_is_the_model_without_the_option():
    plain, _ = tiny_model(dropout=0.1)
    opt, _ = tiny_model(dropout=0.1, mlm_head=True, mlm_weight=0.0, **MLM)
    missing, unexpected = opt.load_state_dict(plain.state_dict(), strict=False)
    assert not unexpected and all(k.startswith("mlm_head.") for k in missing)
    kw, labels = batch()
    a, ga = step(plain.train(), labels, **kw)
    paths_a = step.paths
    b, gb = step(opt.train(), labels, **kw)
    assert torch.equal(a, b) and opt.last_mlm_loss is None
    assert set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    assert paths_a == step.paths


def test_auxiliary_term_adds_weight_times_the_mlm_loss():
    w = 0.25
    plain, _ = tiny_model()
    aux, _ = tiny_model(mlm_weight=w, mlm_probability=0.4, **MLM)
    aux.load_state_dict(plain.state_dict(), strict=False)
    kw, labels = batch()
    nll, _ = step(plain.eval(), labels, **kw)  # eval: no dropout, pass 1 of both models is the same arithmetic
    loss, g = step(aux.eval(), labels, **kw)
    mlm_loss = aux.last_mlm_loss
    assert mlm_loss is not None and bool(torch.isfinite(mlm_loss)) and float(mlm_loss) > 0
    want = float(nll) + w * float(mlm_loss)
    print(f"loss {float(loss):.7f}, nll {float(nll):.7f} + {w} * mlm {float(mlm_loss):.7f} = {want:.7f}")
    assert abs(float(loss) - want) <= 4 * 2.0 ** -24 * abs(want)  # one fp32 product and one fp32 add
    for n in ("mlm_head.predictions.bias", "fc.weight", "bert.embeddings.word_embeddings.weight", "encoder_conv.0.weight"):
        assert float(g[n].abs().max()) > 0, n


@pytest.mark.parametrize("accum", [1, 2])
def test_one_optimizer_step_moves_the_bias_and_the_tied_table(accum):
    from mtvaf_amd.optim import build_optimizer, reference_param_groups
    m, args = tiny_model(mlm_weight=0.5, mlm_probability=0.4, gradient_accumulation_steps=accum, **MLM)
    m.train()
    opt, sched = build_optimizer(m, args, 10)
    listed = reference_param_groups(m, args.lr, True)  # (what build_optimizer hands to AdamW for these args)
    groups = {id(p): (g["lr"], g["weight_decay"]) for g in listed for p in g["params"]}
    named = dict(m.named_parameters())
    assert len(groups) == sum(len(g["params"]) for g in listed)  # every parameter once, the tied table included
    assert groups[id(named["mlm_head.predictions.transform.dense.weight"])] == (5e-2, 1e-2)
    for n in ("mlm_head.predictions.bias", "mlm_head.predictions.transform.dense.bias", "mlm_head.predictions.transform.LayerNorm.weight",
              "mlm_head.predictions.transform.LayerNorm.bias"):
        assert groups[id(named[n])] == (5e-2, 0.0), n
    assert groups[id(named["bert.embeddings.word_embeddings.weight"])] == (1e-3, 1e-2)
    assert m.mlm_head.predictions.decoder.weight is named["bert.embeddings.word_embeddings.weight"]
    kw, labels = batch()
    before = {n: named[n].detach().clone() for n in ("mlm_head.predictions.bias", "bert.embeddings.word_embeddings.weight",
                                                     "bert.encoder.layer.0.attention.self.query.weight")}
    opt.zero_grad(set_to_none=True)
    for _ in range(accum):
        (m(labels=labels, **kw).loss / accum).backward()
    # the table's gradient holds the decoder's share: rows of ids that are not in the batch are touched by the decoder only
    absent = torch.ones(CFG.vocab_size, dtype=torch.bool, device=DEV)
    absent[kw["input_ids"].unique()] = False
    absent[MLM["mlm_mask_token_id"]] = False
    g_table = named["bert.embeddings.word_embeddings.weight"].grad
    assert bool(absent.sum() > 300) and bool((g_table[absent].abs().amax(1) > 0).all())
    opt.step()
    sched.step()
    torch.cuda.synchronize()
    for n, old in before.items():
        new = named[n].detach()
        assert bool(torch.isfinite(new).all()) and not torch.equal(new, old), n
    assert not torch.equal(named["bert.embeddings.word_embeddings.weight"].detach()[absent], before["bert.embeddings.word_embeddings.weight"][absent])
