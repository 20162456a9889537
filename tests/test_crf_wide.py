"""Wide tag sets (17 to 64 tags) on the CPU: the CRF module and TVNetSAModel2 accept them, and the inputs the GPU file
(test_crf_wide_gpu.py) decodes are ones the float32 reference itself ranks within the Viterbi acceptance rule."""
import types

import pytest
import torch
from transformers import BertConfig

import crf_wide_cases as W
from oracle import mtvaf_oracle as O

# the BIOES polarity tag set of the reference's TVSAProcessor.get_label_mapping (16 labels; the model adds one tag)
BIOES_LABELS = ["O", "EQ", "B-POS", "I-POS", "E-POS", "S-POS", "B-NEG", "I-NEG", "E-NEG", "S-NEG", "B-NEU", "I-NEU",
                "E-NEU", "S-NEU", "[CLS]", "[SEP]"]


@pytest.mark.parametrize("C", [17, 21, 33, 64])
def test_crf_module_builds_wide_tag_sets(C):
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(C, batch_first=True)
    assert crf.num_tags == C
    assert tuple(crf.start_transitions.shape) == (C,) and tuple(crf.end_transitions.shape) == (C,)
    assert tuple(crf.transitions.shape) == (C, C)


def test_crf_module_rejects_unsupported_tag_counts():
    from mtvaf_amd.modules.crf import CRF
    with pytest.raises(NotImplementedError, match="64"):
        CRF(65)
    with pytest.raises(ValueError):
        CRF(0)


def test_tvnet2_builds_with_the_bioes_label_set():
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = BertConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", bert_config=cfg, use_prefix=True, vao=False,
                                 noauxloss=True, use_probe=False, n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768,
                                 device="cpu", resnet_root=None, use_152=False)
    m = TVNetSAModel2(BIOES_LABELS, None, args)
    assert m.crf.num_tags == m.fc.out_features == 17


def _fp32_decode(inputs):
    em, _, mask, start, end, trans = inputs
    return O.crf_decode(em, mask, start, end, trans)


@pytest.mark.parametrize("B,S,C,scale", W.FIXED)
def test_fixed_cases_float32_reference_meets_the_viterbi_rule(B, S, C, scale):
    inputs = W.fixed_case(B, S, C, scale)
    em, _, mask, start, end, trans = inputs
    near, bad = W.viterbi_near_ties(_fp32_decode(inputs), em, mask, start, end, trans)
    assert not bad and near <= W.viterbi_cap(B), (near, bad)


def test_random_draws_float32_reference_meets_the_viterbi_rule():
    near_total, n = 0, 0
    for tag, inputs in W.random_draws():
        em, _, mask, start, end, trans = inputs
        near, bad = W.viterbi_near_ties(_fp32_decode(inputs), em, mask, start, end, trans)
        assert not bad, (tag, bad)
        near_total += near
        n += em.shape[0]
    assert near_total <= W.viterbi_cap(n), (near_total, n)


@pytest.mark.parametrize("B,S,C,seed,lengths", W.BRUTE)
def test_bruteforce_cases_float32_reference_is_exact(B, S, C, seed, lengths):
    em, _, mask, start, end, trans = W.crf_inputs(B, S, C, seed, lengths=lengths)
    _, best = O.crf_bruteforce(em, mask, start, end, trans)
    assert O.crf_decode(em, mask, start, end, trans) == best
