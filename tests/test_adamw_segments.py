"""Host logic of the segmented AdamW path (no GPU): the plan builder ``optim.layer_segments``, the fine-tuning recipe
``optim.finetune_param_groups`` on a tiny TVNetSAModel2, and ``build_optimizer``'s defaults."""
import re
import types

import pytest
import torch

LABELS = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]
LAYERS = 3


def _h(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8):
    return dict(lr=lr, weight_decay=wd, betas=betas, eps=eps)


# ---- layer_segments -----------------------------------------------------------------------------------------------------
def test_offsets_out_of_order_are_sorted_and_adjacent_equal_hypers_merge():
    from mtvaf_amd.optim import layer_segments
    a, b = _h(wd=1e-2), _h(wd=0.0)
    #          tensor:  0      1      2     3      4   (given out of buffer order)
    offsets = [8, 0, 20, 24, 12]
    numels = [4, 8, 4, 7, 8]
    hypers = [a, a, b, b, dict(a)]  # (tensor 4 carries an equal copy, not the same object)
    plan = layer_segments(offsets, numels, hypers)
    # buffer order: 1 (a) 0 (a) 4 (a copy) | 2 (b) 3 (b)
    assert [e for e, _ in plan] == [20, 31]
    assert plan[0][1] is a and plan[1][1] is b
    # by identity (what the optimizer asks for: equal values today need not stay equal under a scheduler) the copy stands alone
    assert [e for e, _ in layer_segments(offsets, numels, hypers, same=lambda x, y: x is y)] == [12, 20, 31]
    # lr alone separates too
    assert [e for e, _ in layer_segments([0, 4], [4, 4], [_h(lr=1e-3), _h(lr=2e-3)])] == [4, 8]
    assert [e for e, _ in layer_segments([0, 4], [4, 4], [_h(), _h()])] == [8]


def test_what_one_launch_cannot_do_gives_none():
    from mtvaf_amd.optim import layer_segments
    a, b = _h(wd=1e-2), _h(wd=0.0)
    assert layer_segments([0, 4], [4, 4], [a, _h(wd=0.0, betas=(0.8, 0.999))]) is None
    assert layer_segments([0, 4], [4, 4], [a, _h(wd=0.0, betas=(0.9, 0.99))]) is None
    assert layer_segments([0, 4], [4, 4], [a, _h(wd=0.0, eps=1e-6)]) is None
    assert layer_segments([0, 4], [4, 4], [a, _h(betas=(0.8, 0.999))]) is None  # (also where lr and weight decay agree)
    assert layer_segments([0, 6], [6, 6], [a, b]) is None          # an inner end of 6
    assert layer_segments([0, 6], [6, 6], [a, a]) == [(12, a)]     # ... which is no end once the two merge
    assert layer_segments([0, 8], [8, 5], [a, b]) == [(8, a), (13, b)]  # the last end may be anything
    assert layer_segments([0, 8], [4, 4], [a, b]) is None          # a gap
    assert layer_segments([4, 8], [4, 4], [a, b]) is None          # does not start at 0
    assert layer_segments([0, 2], [4, 4], [a, b]) is None          # overlap
    assert layer_segments([], [], []) is None


def test_sixteen_distinct_tensors_give_sixteen_segments_and_seventeen_none():
    from mtvaf_amd.optim import MAX_SEGMENTS, layer_segments
    hs = [_h(lr=1e-3 * (i + 1)) for i in range(17)]
    plan = layer_segments([4 * i for i in range(16)], [4] * 16, hs[:16])
    assert MAX_SEGMENTS == 16 and [e for e, _ in plan] == [4 * (i + 1) for i in range(16)]
    assert all(h is hs[i] for i, (_, h) in enumerate(plan))
    assert layer_segments([4 * i for i in range(17)], [4] * 17, hs) is None


# ---- finetune_param_groups ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from transformers import BertConfig
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=True, vao=False, noauxloss=True, use_probe=False, n_gpu=1,
                                 alpha=0.0, beta=0.0, prefix_len=4, prefix_dim=768, device="cpu", resnet_root=None, use_152=False)
    args.bert_config = BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=LAYERS, num_attention_heads=1, intermediate_size=128,
                                  max_position_embeddings=16, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    return TVNetSAModel2(LABELS, None, args)


def _ids(groups):
    return [[id(p) for p in g["params"]] for g in groups]


def test_every_parameter_of_the_reference_groups_appears_exactly_once(model):
    from mtvaf_amd.optim import finetune_param_groups, reference_param_groups
    for use_prefix in (True, False):
        ref = [i for g in _ids(reference_param_groups(model, 1e-3, use_prefix)) for i in g]
        got = [i for g in _ids(finetune_param_groups(model, 1e-3, layer_lr_decay=0.8, use_prefix=use_prefix)) for i in g]
        assert len(got) == len(set(got)) and sorted(got) == sorted(ref)
    names = {id(p): n for n, p in model.named_parameters()}
    got = {names[i] for g in _ids(finetune_param_groups(model, 1e-3)) for i in g}
    assert any(n.startswith("projectors.") for n in names.values())
    assert not any(n.startswith("projectors.") or "img_classifier" in n for n in got)  # the reference's quirk is kept


def test_no_decay_names_carry_weight_decay_zero_and_the_lr_follows_the_depth(model):
    from mtvaf_amd.optim import finetune_param_groups
    lr, d, wd = 2e-3, 0.5, 0.03
    names = {id(p): n for n, p in model.named_parameters()}
    groups = finetune_param_groups(model, lr, weight_decay=wd, layer_lr_decay=d, head_lr=7e-2)
    seen = 0
    for g in groups:
        assert g["params"], "no empty group beside a populated one"
        for p in g["params"]:
            n = names[id(p)]
            seen += 1
            exempt = "bias" in n or "LayerNorm.weight" in n
            assert g["weight_decay"] == (0.0 if exempt else wd), n
            m = re.search(r"encoder\.layer\.(\d+)\.", n)
            if n.startswith("crf") or n.startswith("fc"):
                want = 7e-2
            elif m:
                want = lr * d ** (LAYERS - 1 - int(m.group(1)))
            elif "bert" in n and "embeddings." in n:
                want = lr * d ** LAYERS
            else:
                want = lr  # the pooler, encoder_conv
            assert g["lr"] == want, (n, g["lr"], want)
    assert seen > 16 * LAYERS
    # the last layer trains at lr itself, every layer holds exactly two groups, and a custom name test is honoured
    by_layer = {}
    for gi, g in enumerate(groups):
        for p in g["params"]:
            m = re.search(r"encoder\.layer\.(\d+)\.", names[id(p)])
            if m:
                by_layer.setdefault(int(m.group(1)), set()).add(gi)
    assert sorted(by_layer) == list(range(LAYERS)) and all(len(s) == 2 for s in by_layer.values())
    only_ln = finetune_param_groups(model, lr, no_decay=("LayerNorm",))
    for g in only_ln:
        for p in g["params"]:
            assert (g["weight_decay"] == 0.0) == ("LayerNorm" in names[id(p)])


def test_without_exemptions_and_depth_decay_the_groups_are_the_reference_groups(model):
    from mtvaf_amd.optim import finetune_param_groups, reference_param_groups
    for use_prefix in (True, False):
        ref = reference_param_groups(model, 3e-3, use_prefix)
        got = finetune_param_groups(model, 3e-3, no_decay=(), layer_lr_decay=1.0, use_prefix=use_prefix)
        assert _ids(got) == _ids(ref)
        for a, b in zip(got, ref):
            assert a["lr"] == b["lr"] and a["weight_decay"] == b.get("weight_decay", 1e-2)  # (1e-2: AdamW's default)
        if use_prefix:
            assert all(set(a) == set(b) for a, b in zip(got, ref))


def test_build_optimizer_defaults_build_todays_groups_and_the_switches_build_the_recipe(model):
    from mtvaf_amd.optim import DEFAULT_NO_DECAY, build_optimizer, finetune_param_groups, reference_param_groups
    frozen = [p for n, p in model.named_parameters() if "image_model" in n]
    try:
        for use_prefix in (True, False):
            args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=use_prefix)
            opt, _ = build_optimizer(model, args, 10)
            ref = reference_param_groups(model, 1e-3, use_prefix)
            assert _ids(opt.param_groups) == _ids(ref)
            for g, r in zip(opt.param_groups, ref):
                assert g["lr"] == r["lr"] and g["weight_decay"] == r.get("weight_decay", 1e-2)
            # explicit "off" values are the defaults
            args.no_decay, args.layer_lr_decay = False, 1.0
            assert _ids(build_optimizer(model, args, 10)[0].param_groups) == _ids(ref)
        args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, no_decay=True, layer_lr_decay=0.9)
        opt, _ = build_optimizer(model, args, 10)
        want = finetune_param_groups(model, 1e-3, no_decay=DEFAULT_NO_DECAY, layer_lr_decay=0.9)
        assert _ids(opt.param_groups) == _ids(want)
        assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(g["lr"], g["weight_decay"]) for g in want]
        args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, no_decay=("LayerNorm",))
        opt, _ = build_optimizer(model, args, 10)
        assert _ids(opt.param_groups) == _ids(finetune_param_groups(model, 1e-3, no_decay=("LayerNorm",)))
    finally:
        for p in frozen:
            p.requires_grad = True
