"""CPU checks of the masked-LM feature: the NumPy restatements of tests/mlm_cases.py against plain float64 formulas, the chunked
recurrence against the one-shot form (ties across a chunk boundary included), and the parameter names of the head and model
against the reference's state_dict keys recorded in tests/golden/mlm_state_keys.json."""
import json
import os

import numpy as np

import mlm_cases as M

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_mask_rule_restatement():
    V, p = 50, 0.5
    ids = np.array([[2, 7, 8, 9, 3, 0], [2, 11, 3, 0, 0, 0]])
    att = (ids != 0).astype(np.int64)
    u = np.zeros((2, 6, 3), dtype=np.float32)
    u[..., 0] = 0.9                      # nobody selected ...
    u[0, 1] = (0.1, 0.5, 0.0)            # ... but: -> [MASK]
    u[0, 2] = (0.1, 0.85, 0.999999)      # -> random id min(V - 1, int(u2 V)) = 49
    u[0, 3] = (0.1, 0.95, 0.3)           # -> unchanged, still predicted
    u[0, 4] = (0.1, 0.5, 0.0)            # [SEP] = 3: special, never selected
    u[1, 1] = (0.5, 0.5, 0.0)            # u0 == p: not selected (strict <)
    u[1, 4] = (0.0, 0.0, 0.0)            # padding
    out, pos, lab, count, stats = M.mask_reference(ids, att, u, p, 4, V, special_ids=(2, 3, 0))
    assert out.tolist() == [[2, 4, 49, 9, 3, 0], [2, 11, 3, 0, 0, 0]]
    assert count == 3 and pos[:3].tolist() == [1, 2, 3] and lab[:3].tolist() == [7, 8, 9]
    assert (pos[3:] == -1).all() and (lab[3:] == -100).all() and stats.tolist() == [4, 3, 0]
    # capacity 2: the third selected token stays as it is and is counted as dropped
    out, pos, lab, count, stats = M.mask_reference(ids, att, u, p, 4, V, special_ids=(2, 3, 0), capacity=2)
    assert out[0].tolist() == [2, 4, 49, 9, 3, 0] and count == 2 and pos.tolist() == [1, 2] and stats.tolist() == [4, 3, 1]
    # a special_mask takes a token out; a non-prefix attention mask is honoured
    sm = np.zeros_like(ids)
    sm[0, 1] = 1
    att2 = att.copy()
    att2[0, 2] = 0
    out, pos, lab, count, stats = M.mask_reference(ids, att2, u, p, 4, V, special_ids=(2, 3, 0), special_mask=sm)
    assert count == 1 and pos[0] == 3 and out[0].tolist() == ids[0].tolist() and stats.tolist() == [2, 1, 0]


def test_ce_restatement_against_plain_float64():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((6, 37)) * 3
    labels = np.array([0, 36, 5, -100, 40, 7])
    ref = M.ce_oneshot(z, labels, 5)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    want = [-np.log(p[0, 0]), -np.log(p[1, 36]), -np.log(p[2, 5]), 0.0, 0.0, 0.0]  # ignored, out of range, beyond count
    np.testing.assert_allclose(ref["loss_row"], want, rtol=1e-12, atol=1e-12)
    assert ref["live"] == 3 and abs(ref["loss"] - sum(want) / 3) < 1e-12
    assert abs(M.ce_oneshot(z, labels, 5, "sum")["loss"] - sum(want)) < 1e-12
    assert M.ce_oneshot(z, labels, 0)["loss"] == 0.0
    g = M.ce_grad_logits(z, labels, 5, np.full(6, 1 / 3))
    eps = 1e-6
    zz = z.copy()
    zz[1, 4] += eps
    assert abs((M.ce_oneshot(zz, labels, 5)["loss"] - ref["loss"]) / eps - g[1, 4]) < 1e-6
    assert not g[3:].any()


def test_chunked_equals_oneshot_with_ties_across_chunks():
    rng = np.random.default_rng(1)
    R, V = 9, 1037
    z = rng.standard_normal((R, V)) * 2
    z[0] *= 5e3                                  # +-1e4 scale
    z[1, [100, 600]] = z[1].max() + 1.0          # an exact tie that straddles chunks: the lower index wins
    z[2, [31, 32]] = z[2].max() + 2.0            # adjacent columns on a 32-boundary
    z[3, 1036] = z[3].max() + 1.0                # the maximum in the last, partial chunk
    labels = np.array([3, 600, 32, 1036, 0, V - 1, 1030, -100, V])
    one = M.ce_oneshot(z, labels, 8)
    assert one["argmax"][1] == 100 and one["argmax"][2] == 31 and one["argmax"][3] == 1036
    for chunk in (32, 256, 1024, V, 4 * V):
        got = M.ce_chunked(z, labels, 8, chunk)
        assert np.isfinite(got["loss_row"]).all()
        np.testing.assert_array_equal(got["argmax"], one["argmax"])
        np.testing.assert_allclose(got["lse_row"], one["lse_row"], rtol=1e-13, atol=1e-12)
        np.testing.assert_allclose(got["loss_row"], one["loss_row"], rtol=1e-12, atol=1e-11)
        assert got["live"] == one["live"] == 7 and got["correct"] == one["correct"]
        assert abs(got["loss"] - one["loss"]) <= 1e-12 * abs(one["loss"])
    assert one["correct"] == 1  # row 3 only: rows 1 and 2 are labelled with the LATER index of their tie


def test_parameter_names_match_the_reference():
    from transformers import BertConfig, RobertaConfig
    from mtvaf_amd.models.modeling_bert import BertForMaskedLM
    from mtvaf_amd.models.modeling_roberta import RobertaForMaskedLM
    from mtvaf_amd.modules.mlm_head import MaskedLMHead
    keys = json.load(open(os.path.join(GOLDEN, "mlm_state_keys.json")))
    kw = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
              max_position_embeddings=64)
    m = BertForMaskedLM(BertConfig(**kw))
    assert sorted(k for k in m.state_dict() if "position_ids" not in k) == keys["BertForMaskedLM"]
    assert sorted(MaskedLMHead(BertConfig(**kw)).state_dict()) == sorted(keys["head"])
    # tied: one Parameter, listed once
    assert m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    assert m.cls.predictions.decoder.bias is m.cls.predictions.bias
    names = [n for n, _ in m.named_parameters()]
    assert "cls.predictions.decoder.weight" not in names and "bert.embeddings.word_embeddings.weight" in names
    assert BertForMaskedLM(BertConfig(**kw), tie=False).cls.predictions.decoder.weight is not m.bert.embeddings.word_embeddings.weight
    r = RobertaForMaskedLM(RobertaConfig(pad_token_id=1, **kw))
    assert sorted(k for k in r.state_dict() if k.startswith("lm_head.")) == sorted(
        "lm_head." + k for k in ("bias", "dense.weight", "dense.bias", "layer_norm.weight", "layer_norm.bias", "decoder.weight",
                                 "decoder.bias"))
    assert r.lm_head.decoder.weight is r.roberta.embeddings.word_embeddings.weight


def test_default_capacity():
    from mtvaf_amd.mlm import default_capacity
    assert default_capacity(32 * 128, 0.15) == 1248  # ceil(2 * 0.15 * 4096) = 1229 -> 1248
    assert default_capacity(48, 0.15) == 32 and default_capacity(10, 0.5) == 10 and default_capacity(40, 1.0) == 40


def test_optimizer_groups_of_the_head():
    """The head's dense weight at the head lr with weight decay, its LayerNorm and biases at the head lr without, the tied table
    once and with the encoder; a model without the option keeps the groups it had."""
    import types
    from transformers import BertConfig
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    from mtvaf_amd.optim import finetune_param_groups, reference_param_groups

    def model(**kw):
        args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=True, vao=False, noauxloss=True, use_probe=False,
                                     n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768, device="cpu", resnet_root=None, use_152=False,
                                     **kw)
        args.bert_config = BertConfig(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      intermediate_size=256, max_position_embeddings=64)
        return TVNetSAModel2(["O", "B", "I"], None, args)

    plain, m = model(), model(mlm_head=True, mlm_mask_token_id=4, mlm_special_ids=(0, 1, 2, 3, 4))
    assert not hasattr(plain, "mlm_head") and plain.mlm_opt["head"] is False
    named = dict(m.named_parameters())
    table = named["bert.embeddings.word_embeddings.weight"]
    assert m.mlm_head.predictions.decoder.weight is table and "mlm_head.predictions.decoder.weight" not in named
    shape = lambda groups: [(g["lr"], g["weight_decay"], len(g["params"])) for g in groups]
    for make in (lambda x: reference_param_groups(x, 1e-3), lambda x: finetune_param_groups(x, 1e-3)):
        groups = make(m)
        where = {id(p): (g["lr"], g["weight_decay"]) for g in groups for p in g["params"]}
        assert len(where) == sum(len(g["params"]) for g in groups)  # nothing listed twice
        assert where[id(named["mlm_head.predictions.transform.dense.weight"])] == (5e-2, 1e-2)
        for n in ("predictions.bias", "predictions.transform.dense.bias", "predictions.transform.LayerNorm.weight",
                  "predictions.transform.LayerNorm.bias"):
            assert where[id(named["mlm_head." + n])] == (5e-2, 0.0), n
        assert where[id(table)][0] == 1e-3
    assert shape(reference_param_groups(plain, 1e-3)) == [(1e-3, 1e-2, 39), (1e-3, 1e-2, 4), (5e-2, 1e-2, 5)]
    with __import__("pytest").raises(ValueError):
        model(mlm_head=True, mlm_mask_token_id=4000)
