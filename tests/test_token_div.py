"""Token-level divergence and the chain-level identity, the parts that need no GPU: the soundness of the float64 restatement the
GPU tests compare against (token_div_cases.py), the identity behind CRF.symmetric_kl by enumeration, and the C-ABI / Python
surface."""
import ctypes
import inspect
import math

import pytest
import torch

import abi_header
import token_div_cases as T

SMALL = [s for s in T.SHAPES if s[0] <= 257]


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_restatement_is_nonnegative_and_js_is_bounded(shape, kind):
    for s in (1.0, 3.0, 40.0):
        x, y = T.make_logits(*shape, s=s)
        rows = T.row_values(x, y, kind)
        assert bool(torch.isfinite(rows).all()) and float(rows.min()) >= -1e-15
        if kind == "js":
            assert float(rows.max()) <= math.log(2.0) * (1 + 1e-12)
    if shape[1] == 1:
        assert float(rows.abs().max()) == 0.0          # one tag: both distributions are the point mass


@pytest.mark.parametrize("kind", T.KINDS)
def test_restatement_is_zero_for_equal_inputs_and_shift_invariant(kind):
    x, y = T.make_logits(65, 11)
    assert float(T.row_values(x, x, kind).abs().max()) <= 1e-15
    rows = T.row_values(x, y, kind, 0.5)
    g = torch.Generator().manual_seed(3)
    sx, sy = 5 * torch.randn(65, 1, generator=g).double(), 5 * torch.randn(65, 1, generator=g).double()
    moved = T.row_values(x.double() + sx, y.double() + sy, kind, 0.5)
    assert float((moved - rows).abs().max()) <= 1e-12 * max(1.0, float(rows.max()))
    # symmetric in its arguments
    assert float((T.row_values(y, x, kind, 0.5) - rows).abs().max()) <= 1e-14 * max(1.0, float(rows.max()))


@pytest.mark.parametrize("kind", T.KINDS)
def test_restatement_reductions_and_masks(kind):
    x, y = T.make_logits(65, 11)
    rows = T.row_values(x, y, kind)
    mask = T.make_mask("prefix", 65)
    live = mask != 0
    assert 0 < int(live.sum()) < 65
    loss, rw = T.token_div_ref(x, y, mask, kind)
    assert abs(float(loss) - float(rows[live].mean())) <= 1e-14 and not bool(rw[~live].any())
    loss_b, _ = T.token_div_ref(x, y, mask, kind, reduction="batch_mean", B=5, scale=0.25)
    assert abs(float(loss_b) - 0.25 * float(rows[live].sum()) / 5) <= 1e-14
    # NaN / inf in the masked rows reach neither the value nor a gradient
    xn, yn = x.clone(), y.clone()
    xn[~live], yn[~live] = float("nan"), float("inf")
    got = T.ref_with_grads(xn, yn, mask, kind)
    want = T.ref_with_grads(x, y, mask, kind)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert not bool(got[2][~live].any()) and not bool(got[3][~live].any())
    # no live row: 0 and zero gradients
    dead = T.ref_with_grads(x, y, T.make_mask("dead", 65), kind)
    assert float(dead[0]) == 0.0 and not bool(dead[2].any()) and not bool(dead[3].any())


def test_restatement_gradients_are_the_documented_formulas():
    x, y = T.make_logits(7, 63)
    for kind in T.KINDS:
        temp = 0.5
        _, _, gx, gy = T.ref_with_grads(x, y, None, kind, temp)
        lp, lq = torch.log_softmax(x.double() / temp, -1), torch.log_softmax(y.double() / temp, -1)
        p, q = lp.exp(), lq.exp()
        if kind == "sym_kl":
            d = lp - lq
            du = 0.5 * (p * (d - (p * d).sum(-1, keepdim=True)) + p - q)
            dv = 0.5 * (q * (-d - (q * -d).sum(-1, keepdim=True)) + q - p)
        else:
            lm = torch.logaddexp(lp, lq) - math.log(2.0)
            a, b = lp - lm, lq - lm
            du = 0.5 * p * (a - (p * a).sum(-1, keepdim=True))
            dv = 0.5 * q * (b - (q * b).sum(-1, keepdim=True))
        g = T.UPSTREAM / temp / 7
        assert float((gx - g * du).abs().max()) <= 1e-13 and float((gy - g * dv).abs().max()) <= 1e-13


def test_extreme_logits_have_a_finite_float64_value():
    x, y = T.extreme_logits()
    sk, js = T.row_values(x, y, "sym_kl"), T.row_values(x, y, "js")
    assert bool(torch.isfinite(sk).all()) and float(sk[0]) > 1e3 and float(sk[-1]) == 0.0
    assert float(js.max()) <= math.log(2.0) * (1 + 1e-12) and abs(float(js[0]) - math.log(2.0)) <= 1e-12


def test_chain_symmetric_kl_identity_by_enumeration():
    """KL(a||b) + KL(b||a) = E_a[sum_t D[t,y_t]] - E_b[sum_t D[t,y_t]] with D = em_a - em_b under shared transitions: both logZ
    cancel.  C = 3, S = 4, B = 2, ragged prefix mask, every path."""
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    em_a, em_b = 2 * rnd(2, 4, 3), 2 * rnd(2, 4, 3)
    kl, ident = T.chain_sym_kl_bruteforce(em_a, em_b, rnd(3), rnd(3), rnd(3, 3), [4, 2])
    assert float(kl.min()) > 1e-3
    assert float((kl - ident).abs().max()) <= 1e-12
    same, ident0 = T.chain_sym_kl_bruteforce(em_a, em_a, rnd(3), rnd(3), rnd(3, 3), [4, 2])
    assert float(same.abs().max()) == 0.0 and float(ident0.abs().max()) == 0.0


def test_symbols_are_declared_bound_and_exported():
    from mtvaf_amd import hip
    from mtvaf_amd.build import SOURCES, build_library
    assert "consistency.hip" in SOURCES
    declared = {name for _, name, _ in abi_header.prototypes()}
    lib = ctypes.CDLL(build_library(verbose=False))
    for name in ("mtvaf_token_divergence_fwd", "mtvaf_token_divergence_bwd"):
        assert name in declared, f"{name} is not declared in include/mtvaf_hip.h"
        assert name in hip.exported_symbols()
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    for fn in ("token_divergence_fwd", "token_divergence_bwd"):
        assert callable(getattr(hip, fn))


def test_python_surface_has_the_documented_signatures():
    from mtvaf_amd import engine
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    from mtvaf_amd.modules.crf import CRF
    fwd = inspect.signature(engine.TokenDivergenceFunction.forward)
    assert list(fwd.parameters) == ["ctx", "x", "y", "mask", "kind", "temperature", "reduction", "scale"]
    sk = inspect.signature(CRF.symmetric_kl)
    assert list(sk.parameters) == ["self", "emissions_a", "emissions_b", "mask", "reduction"]
    assert sk.parameters["reduction"].default == "mean" and "logZ" in CRF.symmetric_kl.__doc__
    plain = inspect.signature(TVNetSAModel2.forward).parameters
    both = inspect.signature(TVNetSAModel2.forward_consistent).parameters
    assert list(both) == list(plain) + ["return_parts"] and both["return_parts"].default is False
    assert all(both[n].default == plain[n].default for n in plain if n != "self")


@pytest.mark.parametrize("name,value", [("consistency_level", "tokens"), ("consistency_kind", "kl"),
                                        ("consistency_aug", "cutoff"), ("consistency_temperature", 0.0)])
def test_misspelt_options_raise_at_construction(name, value):
    import types
    from mtvaf_amd.models import bert_model
    with pytest.raises(ValueError, match=name):
        bert_model._consistency_options(types.SimpleNamespace(**{name: value}))
    src = inspect.getsource(bert_model.TVNetSAModel2.__init__)
    assert "_consistency_options(args)" in src
