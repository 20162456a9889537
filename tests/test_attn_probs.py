"""Attention probabilities on request (output_attentions), the part that needs no GPU: the C ABI of the new entry points
and the two ``args`` switches of the drop-in models."""
import ctypes
import types

import pytest

import abi_header


@pytest.mark.parametrize("name,nargs", [("mtvaf_prefix_attn_probs", 12), ("mtvaf_prefix_attn_mass", 11)])
def test_header_declares_the_symbol_and_the_binding_matches(name, nargs):
    from mtvaf_amd import hip
    res, _, args = abi_header.prototype(name)
    assert res == "int" and len(args) == nargs, args
    assert name in hip.exported_symbols()
    restype, argtypes = hip._SIGS[name]
    assert restype is ctypes.c_int
    assert list(argtypes) == abi_header.signature(name)[1], (args, argtypes)
    # B, S, P, NH, head_dim, zero_masked_queries, stream close the list
    assert [a for _, a in args[-7:]] == ["B", "S", "P", "NH", "head_dim", "zero_masked_queries", "stream"]


def test_library_exports_the_symbols():
    from mtvaf_amd.build import build_library
    lib = ctypes.CDLL(build_library(verbose=False))
    assert hasattr(lib, "mtvaf_prefix_attn_probs") and hasattr(lib, "mtvaf_prefix_attn_mass")


def test_argument_checks_come_before_any_launch():
    """The header's convention: a negative code for head_dim != 64, a null output, non-positive dimensions (host-side tests:
    nothing is launched, so this runs without a GPU)."""
    from mtvaf_amd import hip
    from mtvaf_amd.build import build_library
    lib = ctypes.CDLL(build_library(verbose=False))
    fn = lib.mtvaf_prefix_attn_probs
    fn.restype, fn.argtypes = hip._SIGS["mtvaf_prefix_attn_probs"]
    x = ctypes.c_void_p(64)  # (never dereferenced: every call below is refused)
    assert fn(x, x, x, x, None, 2, 16, 4, 2, 32, 0, None) < 0      # head_dim
    assert fn(x, x, x, None, None, 2, 16, 4, 2, 64, 0, None) < 0    # probs == NULL
    assert fn(x, x, x, x, None, 0, 16, 4, 2, 64, 0, None) < 0       # B
    assert fn(x, x, x, x, None, 2, 0, 4, 2, 64, 0, None) < 0        # S
    assert fn(x, x, x, x, None, 2, 16, -1, 2, 64, 0, None) < 0      # P
    assert fn(x, x, x, x, None, 2, 16, 4, 0, 64, 0, None) < 0       # NH
    assert fn(x, None, x, x, None, 2, 16, 4, 2, 64, 0, None) < 0    # P > 0 without a prefix slab
    assert fn(x, x, None, x, None, 2, 16, 4, 2, 64, 0, None) < 0    # no mask
    gn = lib.mtvaf_prefix_attn_mass
    gn.restype, gn.argtypes = hip._SIGS["mtvaf_prefix_attn_mass"]
    assert gn(x, x, x, None, 2, 16, 4, 2, 64, 0, None) < 0          # prefix_mass == NULL
    assert gn(x, x, x, x, 2, 16, 4, 2, 48, 0, None) < 0


def test_output_attentions_selects_layers():
    from mtvaf_amd.models.modeling_bert import _attention_layers
    assert _attention_layers(None, 4) is None and _attention_layers(False, 4) is None
    assert _attention_layers(True, 4) == {0, 1, 2, 3}
    assert _attention_layers([1], 4) == {1} and _attention_layers((0, -1), 4) == {0, 3}
    assert _attention_layers([], 4) == set()
    with pytest.raises(IndexError):
        _attention_layers([4], 4)


def _tiny_config():
    from transformers import BertConfig
    return BertConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                      max_position_embeddings=64, hidden_act="gelu")


def _args(**kw):
    """An ``args`` namespace as the trainer builds it -- WITHOUT output_attentions / output_prefix_mass."""
    base = dict(bert_name="bert-base-uncased", use_prefix=False, vao=False, noauxloss=True, use_probe=False, n_gpu=1, alpha=0.5,
                beta=0.0, prefix_len=4, prefix_dim=768, device="cpu", resnet_root=None, use_152=False, bert_config=_tiny_config())
    base.update(kw)
    return types.SimpleNamespace(**base)


LABELS = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]


class _Asked(Exception):
    pass


def _record_bert_call(model, seen):
    def fake_bert(**kw):
        seen.update(kw, prefix_mass=model.bert.encoder.output_prefix_mass)
        raise _Asked()
    model.bert.forward = fake_bert


def test_tvnet2_reads_both_switches_with_a_false_default():
    """The reference hard-codes output_attentions=True in its self.bert(...) calls; here the flag comes from args through
    getattr with a False default, so a namespace that lacks both switches builds and asks for nothing."""
    import torch
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = _args()
    assert not hasattr(args, "output_attentions") and not hasattr(args, "output_prefix_mass")
    m = TVNetSAModel2(LABELS, None, args)
    assert m.last_prefix_mass is None and m.bert.encoder.output_prefix_mass is False
    ids = torch.ones(2, 8, dtype=torch.long)
    seen = {}
    _record_bert_call(m, seen)
    with pytest.raises(_Asked):
        m(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
    assert seen["output_attentions"] is False and seen["prefix_mass"] is False
    args.output_attentions, args.output_prefix_mass = [1], True  # (read at every forward, not frozen at construction)
    with pytest.raises(_Asked):
        m(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
    assert seen["output_attentions"] == [1] and seen["prefix_mass"] is True


def test_span_model_passes_the_flag_default():
    import torch
    from mtvaf_amd.models.bert_model import TVNetSAModel
    args = _args()
    m = TVNetSAModel(LABELS, None, args)
    ids = torch.ones(2, 8, dtype=torch.long)
    seen = {}
    _record_bert_call(m, seen)
    with pytest.raises(_Asked):
        m._extract(torch.ones_like(ids), ids, None, torch.zeros_like(ids))
    assert seen["output_attentions"] is False
