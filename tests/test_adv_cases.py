"""CPU side of the adversarial step: the float64 restatement of adv_cases.py has the properties the
contract states, the binding and the public module exist without a GPU, and Adversary checks its optimizer.  The kernel itself
is tested on the MI355X (test_adv_gpu.py)."""
import types

import pytest
import torch

import adv_cases as A

IDS = [c["id"] for c in A.CASES]


@pytest.mark.parametrize("scope", A.SCOPES)
@pytest.mark.parametrize("case", A.CASES[:-1], ids=IDS[:-1])
def test_fgm_delta_has_norm_eps_on_live_units_and_zero_on_dead_rows(case, scope):
    g, mask, _ = A.make_inputs(case)
    r = A.reference(g, mask, A.EPS, norm="l2", scope=scope)
    d = r["delta"]
    live = mask.ne(0)
    assert bool((d[~live] == 0).all()), "dead rows are exact zeros"
    n = A.unit_norm(d, scope)[..., 0]
    assert torch.allclose(n[live], torch.full_like(n[live], A.EPS), rtol=1e-12, atol=0)
    for b in range(case["B"]):  # a sentence without a live row: nothing, and its norms are 0
        if not bool(live[b].any()):
            assert float(r["stats"][b, 0]) == 0 and float(r["stats"][b, 1]) == 0 and not bool(d[b].any())
    # Linf: every live element with a gradient sits on the cube's surface, with the gradient's sign
    li = A.reference(g, mask, A.EPS, norm="linf", scope=scope)["delta"]
    assert torch.equal(li, torch.where(live[..., None], A.EPS * torch.sign(g.double()), torch.zeros((), dtype=torch.float64)))


@pytest.mark.parametrize("norm", A.NORMS)
@pytest.mark.parametrize("scope", A.SCOPES)
@pytest.mark.parametrize("case", A.CASES[1:-1], ids=IDS[1:-1])
def test_projection_lands_in_the_ball_and_is_idempotent(case, norm, scope):
    for mode in ("bites", "inside"):
        g, mask, din = A.make_inputs(case, mode)
        live = mask.ne(0)
        d = A.reference(g, mask, A.EPS, A.STEP, norm, scope, delta_in=din)["delta"]
        assert bool((d[~live] == 0).all())
        if norm == "l2":
            n = A.unit_norm(d, scope)[..., 0]
            assert bool((n[live] <= A.EPS * (1 + 1e-12)).all())
            stepped = torch.where(live[..., None], din.double() + A.STEP * (g.double() / A.unit_norm(
                torch.where(live[..., None], g.double(), torch.zeros((), dtype=torch.float64)), scope).clamp_min(1e-300)), torch.zeros((), dtype=torch.float64))
            cut = A.unit_norm(stepped, scope)[..., 0] > A.EPS
            if mode == "inside":
                assert not bool(cut[live].any()) and torch.equal(d, stepped), "the projection leaves a point inside the ball alone"
            elif case["H"] >= 64:
                assert bool(cut[live].all()), "the projection bites"
        else:
            assert float(d.abs().max()) <= A.EPS
        # a zero step from the result is the projection alone: it changes nothing (up to its own float64 rounding)
        again = A.reference(torch.zeros_like(g), mask, A.EPS, A.STEP, norm, scope, delta_in=d)["delta"]
        assert torch.allclose(again, d, rtol=1e-12, atol=0)


@pytest.mark.parametrize("norm", A.NORMS)
@pytest.mark.parametrize("scope", A.SCOPES)
def test_degenerate_units_give_finite_results(norm, scope):
    case = A.CASES[2]
    g, mask, din = A.make_inputs(case, "bites")
    mask[2, :4] = 1     # (the case's dead sentence gets live rows: a sentence whose gradient is all zero)
    g[2] = 0.0
    g[1, 2, 5], g[1, 3, 7] = float("inf"), float("nan")
    g[1, 10] = float("nan")  # a dead row: ignored
    r = A.reference(g, mask, A.EPS, norm=norm, scope=scope)
    assert bool(torch.isfinite(r["delta"]).all())
    assert not bool(r["delta"][2].any()), "zero gradient: zero delta"
    if scope == "sentence":
        assert not bool(r["delta"][1].any()), "a sentence with an inf and a NaN: zero delta"
    else:
        assert not bool(r["delta"][1, 2:4].any()) and bool(r["delta"][1, 0].any()), "only the rows that hold them"
    assert float(r["stats"][2, 0]) == 0 and not bool(torch.isfinite(r["stats"][1, 0])) and bool(torch.isfinite(r["stats"][0, 0]))
    # with delta_in: the projected delta_in, unchanged by the gradient
    p = A.reference(g, mask, A.EPS, A.STEP, norm, scope, delta_in=din)
    alone = A.reference(torch.zeros_like(g), mask, A.EPS, A.STEP, norm, scope, delta_in=din)
    assert bool(torch.isfinite(p["delta"]).all()) and torch.equal(p["delta"][2], alone["delta"][2])
    rows = slice(None) if scope == "sentence" else slice(2, 4)
    assert torch.equal(p["delta"][1, rows], alone["delta"][1, rows])


def test_scale_of_the_gradient_does_not_move_the_reference():
    g, mask, _ = A.make_inputs(A.CASES[4])
    base = A.reference(g, mask, A.EPS)["delta"]
    for k in (-60, 60):
        assert torch.allclose(A.reference(g * 2.0 ** k, mask, A.EPS)["delta"], base, rtol=1e-12, atol=0)
    # what the kernel's double accumulation is for: fp32 squares of a scaled-down gradient are subnormal (a few bits) or gone
    assert float(((g * 1e-3 * 2.0 ** -60) ** 2).sum()) == 0.0


def test_binding_and_public_module_exist_without_a_gpu():
    from mtvaf_amd import hip
    assert {"mtvaf_adv_perturb", "mtvaf_adv_workspace_bytes", "mtvaf_adv_add"} <= set(hip._SIGS)
    import abi_header as H
    for name in ("mtvaf_adv_perturb", "mtvaf_adv_workspace_bytes", "mtvaf_adv_add"):
        assert (hip._SIGS[name][0], list(hip._SIGS[name][1])) == H.signature(name), name
    d = H.defines()
    assert (hip.ADV_NORMS, hip.ADV_SCOPES) == ({"l2": d["MTVAF_ADV_NORM_L2"], "linf": d["MTVAF_ADV_NORM_LINF"]},
                                               {"sentence": d["MTVAF_ADV_SCOPE_SENTENCE"], "token": d["MTVAF_ADV_SCOPE_TOKEN"]})
    lib = hip.lib()  # host-side answers only: no GPU call
    assert lib.mtvaf_adv_workspace_bytes(32, 128) == 32 * 128 * 3 * 8
    assert lib.mtvaf_adv_workspace_bytes(1, 513) == 0 and lib.mtvaf_adv_workspace_bytes(0, 4) == 0
    import mtvaf_amd.adversarial as adv
    assert callable(adv.Adversary) and callable(adv.from_args)
    from mtvaf_amd import engine
    from mtvaf_amd.models.modeling_bert import BertModel
    from mtvaf_amd.models.modeling_roberta import RobertaModel
    assert BertModel.embedding_tap is None and RobertaModel.embedding_tap is None
    tap = engine.EmbeddingTap()
    assert tap.delta is None and tap.capture is False and tap.grad is None


def _stub_model():
    return types.SimpleNamespace(bert=types.SimpleNamespace(embedding_tap=None, encoder=types.SimpleNamespace(_sink=None)))


def test_adversary_checks_its_arguments_and_its_optimizer():
    from mtvaf_amd.adversarial import Adversary, from_args
    m = _stub_model()
    opt = lambda k, overlap=False, graphed=None: types.SimpleNamespace(accumulation_steps=k, overlap=overlap, _graphed=graphed)
    a = Adversary(m, eps=1.0, steps=3)
    assert a.passes == 4 and a.step_size == pytest.approx(1.0 / 3) and a.norm == "l2" and a.scope == "sentence"
    Adversary(m, optimizer=opt(1))          # the fallback
    Adversary(m, optimizer=opt(2))          # fused accumulation over 1 + steps passes
    Adversary(m, steps=2, optimizer=opt(3, overlap=True))
    with pytest.raises(ValueError, match="accumulation_steps=3"):
        Adversary(m, optimizer=opt(3))
    with pytest.raises(ValueError, match="accumulation_steps=2"):
        Adversary(m, steps=2, optimizer=opt(2))
    with pytest.raises(ValueError, match="overlap"):
        Adversary(m, optimizer=opt(1, overlap=True))
    with pytest.raises(RuntimeError, match="GraphedTrainStep"):
        Adversary(m, optimizer=opt(2, graphed=object()))
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(norm="l1"), dict(scope="batch"), dict(steps=0), dict(step_size=-1.0),
                dict(weight=-1.0)):
        with pytest.raises(ValueError):
            Adversary(m, **bad)
    with pytest.raises(ValueError, match="bert"):
        Adversary(types.SimpleNamespace())
    # build_optimizer's arguments: nothing is built at the default
    assert from_args(m, types.SimpleNamespace()) is None and from_args(m, types.SimpleNamespace(adv_eps=0.0)) is None
    b = from_args(m, types.SimpleNamespace(adv_eps=0.5, adv_norm="linf", adv_steps=2, adv_weight=0.5))
    assert (b.eps, b.norm, b.steps, b.weight, b.step_size) == (0.5, "linf", 2, 0.5, 0.25)


def test_adversary_refuses_a_real_optimizer_with_another_pass_count():
    """mtvaf_amd.optim.AdamW(accumulation_steps=3) on a model whose step is 1 + 1 passes; and GradSync's hook on the sink."""
    from mtvaf_amd.adversarial import Adversary
    from mtvaf_amd.optim import AdamW
    from test_accumulation import _Encoder
    m = types.SimpleNamespace(bert=types.SimpleNamespace(embedding_tap=None, encoder=_Encoder()))
    m.bert.encoder.grad_sink = m.bert.encoder._sink
    o = AdamW(list(m.bert.encoder.parameters()), model=m, accumulation_steps=3)
    with pytest.raises(ValueError, match="accumulation_steps=3"):
        Adversary(m, steps=1, optimizer=o)
    a = Adversary(m, steps=2, optimizer=o)
    a._check_sink()
    # an optimizer attached to the encoder without a word to the Adversary is found at step time
    with pytest.raises(ValueError, match="accumulation_steps=3"):
        Adversary(m, steps=1).step(attention_mask=torch.ones(1, 1))
    assert m.bert.embedding_tap is None

    class GradSync:  # (the hook's owner is recognised by its class: no process group here)
        def _layer_done(self, li, flat):
            pass

    m.bert.encoder._sink.on_layer_done = GradSync()._layer_done
    with pytest.raises(RuntimeError, match="GradSync"):
        a.step(attention_mask=torch.ones(1, 1))
    assert m.bert.embedding_tap is None
