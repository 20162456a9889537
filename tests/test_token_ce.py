"""Token cross entropy, the parts that need no GPU: the float64 restatement the GPU tests compare against (token_ce_cases.py)
equals torch.nn.functional.cross_entropy at gamma = 0, the documented gradient formula equals autograd, the edge cases, and the
C-ABI / Python surface."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

import abi_header
import token_ce_cases as T

SMALL = [s for s in T.SHAPES if s[0] <= 257]


@pytest.mark.parametrize("smoothing", T.SMOOTHINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_restatement_equals_torch_cross_entropy_at_gamma_0(shape, weighted, smoothing):
    N, C = shape
    z, labels = T.make_logits(N, C).double(), T.make_labels(N, C)
    weight = T.make_weights(C) if weighted else None
    wd = None if weight is None else weight.double()
    live = T.live_rows(labels, None, C)
    for reduction, torch_reduction in (("mean", "mean"), ("sum", "sum")):
        ref, rows = T.token_ce_ref(z, labels, None, weight, smoothing, 0.0, reduction)
        want = F.cross_entropy(z, labels, weight=wd, ignore_index=T.IGNORE, label_smoothing=smoothing, reduction=torch_reduction)
        if reduction == "mean" and (not bool(live.any()) or (weighted and float(wd[labels[live]].sum()) == 0.0)):
            assert float(ref) == 0.0   # torch divides 0 by 0 here; the contract says 0
            continue
        assert abs(float(ref) - float(want)) <= 1e-13 * max(1.0, abs(float(want))), (float(ref), float(want))
    per_row = F.cross_entropy(z, labels, weight=wd, ignore_index=T.IGNORE, label_smoothing=smoothing, reduction="none")
    assert float((rows - per_row).abs().max()) <= 1e-13 * max(1.0, float(per_row.abs().max()))


def test_masked_rows_are_torchs_ignored_rows():
    N, C = 65, 11
    z, labels, mask, weight = T.make_logits(N, C).double(), T.make_labels(N, C), T.make_mask("prefix", N), T.make_weights(C)
    ref, _ = T.token_ce_ref(z, labels, mask, weight, 0.1, 0.0, "mean")
    folded = torch.where(mask != 0, labels, torch.full_like(labels, T.IGNORE))
    want = F.cross_entropy(z, folded, weight=weight.double(), ignore_index=T.IGNORE, label_smoothing=0.1)
    assert abs(float(ref) - float(want)) <= 1e-13
    # batch_mean and scale
    bm, rows = T.token_ce_ref(z, labels, mask, weight, 0.1, 2.0, "batch_mean", B=5, scale=0.25)
    assert abs(float(bm) - 0.25 * float(rows.sum()) / 5) <= 1e-15


@pytest.mark.parametrize("gamma", T.GAMMAS)
@pytest.mark.parametrize("smoothing", T.SMOOTHINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 11), (5, 17), (65, 11)], ids=str)
def test_documented_gradient_equals_autograd(shape, weighted, smoothing, gamma):
    N, C = shape
    z, labels, mask = T.make_logits(N, C).double().requires_grad_(True), T.make_labels(N, C), T.make_mask("prefix", N)
    weight = T.make_weights(C) if weighted else None
    live = T.live_rows(labels, mask, C)
    rows = T.row_values(z, labels, live, weight, smoothing, gamma)
    (auto,) = torch.autograd.grad(rows.sum(), (z,))
    formula = T.formula_grad(z.detach(), labels, live, weight, smoothing, gamma)
    assert float((auto - formula).abs().max()) <= 1e-13 * max(1.0, float(auto.abs().max()))
    assert not bool(formula[~live].any())


def test_focal_at_gamma_0_is_ce_and_one_tag_is_zero():
    z, labels = T.make_logits(7, 11).double(), T.make_labels(7, 11)
    live = T.live_rows(labels, None, 11)
    plain = T.row_values(z, labels, live)
    lp = torch.log_softmax(z, -1)
    want = -lp[torch.arange(7), labels.clamp(min=0)] * live
    assert float((plain - want).abs().max()) <= 1e-14
    # gamma > 0 scales each row by (1 - p_y)^gamma
    py = lp.exp()[torch.arange(7), labels.clamp(min=0)]
    focal = T.row_values(z, labels, live, gamma=2.0)
    assert float((focal - (1 - py) ** 2 * plain).abs().max()) <= 1e-13
    # one tag: log_softmax is 0, every value and gradient is 0
    z1, y1 = torch.randn(4, 1, dtype=torch.float64), torch.zeros(4, dtype=torch.long)
    for gamma in T.GAMMAS:
        for eps in T.SMOOTHINGS:
            loss, rows = T.token_ce_ref(z1, y1, None, None, eps, gamma)
            assert float(loss) == 0.0 and not bool(rows.any())
            assert not bool(T.formula_grad(z1, y1, torch.ones(4, dtype=torch.bool), None, eps, gamma).any())


def test_nan_in_dead_rows_reaches_nothing_and_no_divisor_gives_zero():
    N, C = 65, 11
    z, labels, mask, weight = T.make_logits(N, C), T.make_labels(N, C), T.make_mask("prefix", N), T.make_weights(C)
    labels[1], labels[2] = C, -1      # out of range: dead
    live = T.live_rows(labels, mask, C)
    assert not bool(live[1]) and not bool(live[2]) and bool(live[0])
    zn = z.clone()
    zn[~live] = float("nan")
    for gamma in (0.0, 2.0):
        a, b = T.ref_with_grads(z, labels, mask, weight, 0.1, gamma), T.ref_with_grads(zn, labels, mask, weight, 0.1, gamma)
        for u, v in zip(a, b):
            assert bool(torch.isfinite(v).all()) and torch.equal(u, v)
        assert not bool(b[2][~live].any())
    # D = 0: no live row, or live rows whose class weights are all 0
    dead = T.make_mask("dead", N)
    loss, rows, gz = T.ref_with_grads(z, labels, dead, weight, 0.1, 2.0)
    assert float(loss) == 0.0 and not bool(rows.any()) and not bool(gz.any())
    w0 = torch.zeros(C)
    loss, rows, gz = T.ref_with_grads(z, labels, mask, w0, 0.0, 0.0)
    assert float(loss) == 0.0 and not bool(gz.any())


def test_symbols_are_declared_bound_and_exported():
    from mtvaf_amd import hip
    from mtvaf_amd.build import SOURCES, build_library
    assert "token_ce.hip" in SOURCES
    declared = {name for _, name, _ in abi_header.prototypes()}
    lib = ctypes.CDLL(build_library(verbose=False))
    for name in ("mtvaf_token_ce_fwd", "mtvaf_token_ce_bwd", "mtvaf_token_argmax"):
        assert name in declared, f"{name} is not declared in include/mtvaf_hip.h"
        assert name in hip.exported_symbols()
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    for fn in ("token_ce_fwd", "token_ce_bwd", "token_argmax"):
        assert callable(getattr(hip, fn))
    assert hip.TOKEN_CE_REDUCTIONS == {"mean": 0, "batch_mean": 1, "sum": 2}


def test_python_surface_has_the_documented_signatures():
    from mtvaf_amd import engine
    from mtvaf_amd.modules.token_head import TokenCrossEntropy
    fwd = inspect.signature(engine.TokenCEFunction.forward)
    assert list(fwd.parameters) == ["ctx", "logits", "labels", "mask", "class_weight", "ignore_index", "smoothing", "gamma",
                                    "reduction", "scale"]
    init = inspect.signature(TokenCrossEntropy.__init__).parameters
    assert list(init) == ["self", "num_tags", "class_weight", "smoothing", "focal_gamma", "ignore_index"]
    assert (init["class_weight"].default, init["smoothing"].default, init["focal_gamma"].default,
            init["ignore_index"].default) == (None, 0.0, 0.0, -100)
    call = inspect.signature(TokenCrossEntropy.forward).parameters
    assert list(call)[:5] == ["self", "logits", "labels", "mask", "reduction"] and call["reduction"].default == "mean"
    assert list(inspect.signature(TokenCrossEntropy.decode).parameters) == ["self", "logits", "mask", "allowed"]
    head = TokenCrossEntropy(11, class_weight=[1.0] * 10 + [0.0], smoothing=0.1, focal_gamma=2.0)
    assert head.last_stats is None and not list(head.parameters()) and head.class_weight.shape == (11,)
    assert TokenCrossEntropy.REDUCTIONS == ("mean", "batch_mean", "sum", "none")
    for bad in (dict(num_tags=65), dict(num_tags=11, smoothing=1.0), dict(num_tags=11, focal_gamma=0.5),
                dict(num_tags=11, focal_gamma=9.0), dict(num_tags=11, class_weight=[1.0] * 10),
                dict(num_tags=2, class_weight=[1.0, -1.0])):
        with pytest.raises(ValueError):
            TokenCrossEntropy(**bad)


@pytest.mark.parametrize("name,value", [("tag_head", "softmx"), ("token_ce_reduction", "none"), ("token_ce_smoothing", 1.0),
                                        ("token_ce_focal_gamma", 0.5), ("token_ce_class_weights", [1.0, 2.0]),
                                        ("token_ce_weight", -1.0)])
def test_misspelt_options_raise_at_construction(name, value):
    import types
    from mtvaf_amd.models import bert_model
    with pytest.raises(ValueError, match=name):
        bert_model._token_head_options(types.SimpleNamespace(**{name: value}), 11)
    assert "_token_head_options(args" in inspect.getsource(bert_model.TVNetSAModel2.__init__)
    opt = bert_model._token_head_options(types.SimpleNamespace(), 11)
    assert opt["head"] == "crf" and opt["weight"] == 0.0 and opt["reduction"] == "batch_mean"
