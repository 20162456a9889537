"""CPU side of the layer mix: the float64 reference of layer_mix_cases.py against central finite
differences of itself (the formula the kernels are held to, not the kernels), the layer selection, the `LayerMix` module and the
optimizer groups."""
import types

import pytest
import torch

import abi_header
import layer_mix_cases as LC


@pytest.mark.parametrize("K,gamma,pattern", [(1, 1.0, "random"), (3, -0.5, "random"), (5, 0.7, "equal"), (4, 0.0, "random")])
def test_reference_gradients_agree_with_finite_differences(K, gamma, pattern):
    gen = torch.Generator().manual_seed(K)
    rows, H = 3, 8
    states = torch.randn(K, rows, H, generator=gen, dtype=torch.float32)
    dy = torch.randn(rows, H, generator=gen, dtype=torch.float32)
    a = LC.make_scalars(K, pattern, gen)
    g = torch.tensor([gamma], dtype=torch.float32)
    ref = LC.reference(states, dy, a, g)
    h64, d64, a64, g64 = states.double(), dy.double(), a.double(), g.double()
    loss = lambda h, a_, g_: float((LC.forward64(h, a_, g_) * d64).sum())
    eps = 1e-6

    def central(make):
        return (loss(*make(+eps)) - loss(*make(-eps))) / (2 * eps)

    tol = lambda x: 1e-7 * (1.0 + float(x.abs().max()))
    fd_gamma = central(lambda e: (h64, a64, g64 + e))
    assert abs(fd_gamma - float(ref["dgamma"])) <= tol(ref["dgamma"])
    for j in range(K):
        unit = torch.zeros(K, dtype=torch.float64)
        unit[j] = 1.0
        fd = central(lambda e: (h64, a64 + e * unit, g64))
        assert abs(fd - float(ref["dscalars"][j])) <= tol(ref["dscalars"]), j
        # d h_j = coef_j * dy, at three elements of every state
        for r, c in ((0, 0), (1, 5), (2, 7)):
            bump = torch.zeros_like(h64)
            bump[j, r, c] = 1.0
            fd = central(lambda e: (h64 + e * bump, a64, g64))
            assert abs(fd - float(ref["coef"][j] * d64[r, c])) <= tol(d64), (j, r, c)
    # the cancellation-free form of d scalars is the one of the issue: gamma s_j (t_j - sum_i s_i t_i)
    s, t = ref["s"], ref["t"]
    assert torch.allclose(ref["dscalars"], g64 * s * (t - (s * t).sum()), rtol=1e-9, atol=1e-12 * float(t.abs().max()))
    assert abs(float(ref["dscalars"].sum())) <= 1e-9 * (1.0 + float(ref["dscalars"].abs().max()))  # (a softmax's gradients add up to 0)


def test_bounds_are_made_from_the_eager_chains_own_error():
    for i in (0, 1, 10):
        ref, bound = LC.bounds(i)
        states, dy, a, g = LC.make_inputs(i)
        eag = LC.eager32(states, dy, a, g)
        for k in ("y", "dh", "dgamma", "dscalars"):  # (the chain against the bound made from it: 1 / FACTOR at the most)
            assert LC.ratio(eag[k], ref[k], bound[k]) <= 1.0 / LC.FACTOR + 1e-12, (i, k)
        assert tuple(ref["dscalars"].shape) == (LC.CASES[i][0],) and tuple(ref["dgamma"].shape) == (1,)
        assert bool((bound["y"] >= 0).all()) and bool((bound["dh"] >= 0).all())


def test_the_case_table_covers_what_the_contract_names():
    ks, rows, hs, pats, gs = (set(c[j] for c in LC.CASES) for j in range(5))
    assert {1, 2, 13, 25, 32} <= ks and {1, 63, 64, 65, 257} <= rows and {64, 768, 1024} <= hs
    assert pats == {"equal", "pm80", "random"} and gs == {1.0, -0.5, 0.0}
    states, dy, a, g = LC.make_inputs(1)
    assert float(a.max()) == 80.0 and float(a.min()) == -80.0
    cls = LC.column_class(64)
    assert float(states[..., cls == 1].abs().max()) < 1e-10 and float(states[..., cls == 2].abs().max()) > 1e5
    d = abi_header.defines()
    assert d["MTVAF_LAYER_MIX_MAX_K"] == 32 == max(ks)
    assert d["MTVAF_LAYER_MIX_WORKSPACE_BYTES"] == 8 * d["MTVAF_LAYER_MIX_MAX_K"] * d["MTVAF_LAYER_MIX_DOT_BLOCKS"]


# ---- the selection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,n,want", [("all", 13, tuple(range(13))), (None, 3, (0, 1, 2)), ([-1], 13, (12,)), ([0, -1], 13, (0, 12)),
                                           ([3, 1, 2], 5, (1, 2, 3)), ((7,), 13, (7,)), ([-13], 13, (0,)), (range(32), 40, tuple(range(32))),
                                           ("all", 32, tuple(range(32)))])
def test_layer_selection_resolves(layers, n, want):
    from mtvaf_amd import engine
    got = engine.resolve_mix_layers(layers, n)
    assert got == want and isinstance(got, tuple)
    if layers is not None:
        assert got == LC.resolve_reference(layers, n)


@pytest.mark.parametrize("layers,n", [([13], 13), ([-14], 13), ([0, 0], 13), ([1, -12], 13), ([], 13), ("all", 33), (range(33), 40),
                                      ("last", 13), ([1.5], 13), (3, 13), ([True], 13)])
def test_layer_selection_raises(layers, n):
    from mtvaf_amd import engine
    with pytest.raises(ValueError):
        engine.resolve_mix_layers(layers, n)


# ---- the module ----------------------------------------------------------------------------------------------------------
def test_module_initialisation_and_weights():
    from mtvaf_amd.modules.layer_mix import LayerMix
    m = LayerMix(13)
    assert m.layers == tuple(range(13)) and m.num_states == 13
    assert set(dict(m.named_parameters())) == {"scalars", "gamma"}
    assert m.scalars.dtype == m.gamma.dtype == torch.float32
    assert tuple(m.scalars.shape) == (13,) and tuple(m.gamma.shape) == (1,)
    assert torch.equal(m.scalars.detach(), torch.zeros(13)) and torch.equal(m.gamma.detach(), torch.ones(1))
    w = m.weights()
    assert not w.requires_grad and w.device == m.scalars.device
    assert torch.allclose(w, torch.full((13,), 1 / 13)) and abs(float(w.sum()) - 1.0) <= 1e-6
    m = LayerMix(13, layers=[0, 6, -1], init_last=3.0)
    assert m.layers == (0, 6, 12) and m.scalars.detach().tolist() == [0.0, 0.0, 3.0]
    w = m.weights()
    e = torch.exp(torch.tensor(3.0))
    assert abs(float(w.sum()) - 1.0) <= 1e-6 and abs(float(w[2]) - float(e / (e + 2))) <= 1e-6
    m = LayerMix(3, layers=[2, 0], init_last=1.0)  # (the LAST chosen state is the highest one, whatever the order given)
    assert m.layers == (0, 2) and m.scalars.detach().tolist() == [0.0, 1.0]
    with pytest.raises(ValueError):
        LayerMix(3, layers=[3])
    with pytest.raises(ValueError):
        LayerMix(40)


class _Toy(torch.nn.Module):
    """The names of a tagger with the option on: an encoder, a head, the mix."""

    def __init__(self):
        super().__init__()
        from mtvaf_amd.modules.layer_mix import LayerMix
        self.bert = torch.nn.Module()
        self.bert.encoder = torch.nn.Module()
        self.bert.encoder.layer = torch.nn.ModuleList([torch.nn.Linear(4, 4) for _ in range(2)])
        self.encoder_conv = torch.nn.Linear(4, 4)
        self.fc = torch.nn.Linear(4, 3)
        self.layer_mix = LayerMix(3)


@pytest.mark.parametrize("use_prefix", [True, False])
@pytest.mark.parametrize("no_decay", ["default", ()])
def test_optimizer_groups_keep_the_mix_out_of_weight_decay(use_prefix, no_decay):
    from mtvaf_amd.optim import DEFAULT_NO_DECAY, finetune_param_groups, reference_param_groups
    m = _Toy()
    mix = {id(m.layer_mix.scalars), id(m.layer_mix.gamma)}
    nd = DEFAULT_NO_DECAY if no_decay == "default" else no_decay
    groups = finetune_param_groups(m, 1e-3, weight_decay=0.01, no_decay=nd, use_prefix=use_prefix, head_lr=5e-2)
    home = [g for g in groups if mix & {id(p) for p in g["params"]}]
    assert len(home) == 1 and mix <= {id(p) for p in home[0]["params"]}, "both parameters, one group"
    assert home[0]["weight_decay"] == 0.0
    assert home[0]["lr"] == (5e-2 if use_prefix else 1e-3)
    if nd:  # the group they share is the no-decay group of their partition: the head's biases sit there too
        assert id(m.fc.bias) in {id(p) for p in home[0]["params"]} and id(m.fc.weight) not in {id(p) for p in home[0]["params"]}
    decayed = [g for g in groups if g["weight_decay"] > 0]
    assert decayed and not any(mix & {id(p) for p in g["params"]} for g in decayed)
    ref = reference_param_groups(m, 1e-3, use_prefix)
    home = [g for g in ref if mix & {id(p) for p in g["params"]}]
    assert len(home) == 1 and home[0]["weight_decay"] == 0.0 and {id(p) for p in home[0]["params"]} == mix
    # every parameter of the toy is in exactly one group (the mix would match no name of the reference's partition)
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen)) == len(list(m.parameters()))


def test_groups_of_a_model_without_the_option_are_what_they_were():
    from mtvaf_amd.optim import finetune_param_groups, reference_param_groups
    m = _Toy()
    m.layer_mix = None
    for use_prefix in (True, False):
        ref = reference_param_groups(m, 1e-3, use_prefix)
        assert len(ref) == (3 if use_prefix else 1)
        fin = finetune_param_groups(m, 1e-3, no_decay=(), use_prefix=use_prefix)
        assert [[id(p) for p in g["params"]] for g in fin] == [[id(p) for p in g["params"]] for g in ref if g["params"] or use_prefix]


def test_binding_declares_the_three_entry_points():
    from mtvaf_amd import hip
    from mtvaf_amd.build import SOURCES
    assert "layermix.hip" in SOURCES
    for name in ("mtvaf_layer_mix_fwd", "mtvaf_layer_mix_dots", "mtvaf_layer_mix_inject"):
        assert (hip._SIGS[name][0], list(hip._SIGS[name][1])) == abi_header.signature(name), name
    d = abi_header.defines()
    assert hip.LAYER_MIX_MAX_K == d["MTVAF_LAYER_MIX_MAX_K"] and hip.LAYER_MIX_WORKSPACE_BYTES == d["MTVAF_LAYER_MIX_WORKSPACE_BYTES"]


def test_models_take_the_option_from_args_and_default_to_nothing():
    """Construction only (no device): args.layer_mix builds the module, None leaves no parameter and no state-dict key."""
    from transformers import BertConfig
    from mtvaf_amd.models.bert_model import TVNetSAModel, TVNetSAModel2
    hf = BertConfig(vocab_size=50, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=32,
                    max_position_embeddings=16)
    labels = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]

    def args(**kw):
        return types.SimpleNamespace(bert_name="bert-base-uncased", bert_config=hf, use_prefix=False, vao=False, noauxloss=True,
                                     use_probe=False, n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768, device="cpu", resnet_root=None,
                                     use_152=False, gcn_layer_number=0, num_layers=0, **kw)
    for cls in (TVNetSAModel2, TVNetSAModel):
        plain = cls(labels, None, args())
        assert plain.layer_mix is None and not any("layer_mix" in k for k in plain.state_dict())
        on = cls(labels, None, args(layer_mix="all", layer_mix_init_last=2.0))
        assert on.layer_mix.layers == (0, 1, 2) and on.layer_mix.scalars.detach().tolist() == [0.0, 0.0, 2.0]
        assert set(on.state_dict()) - set(plain.state_dict()) == {"layer_mix.scalars", "layer_mix.gamma"}
        assert cls(labels, None, args(layer_mix=[-1])).layer_mix.layers == (2,)
        with pytest.raises(ValueError):
            cls(labels, None, args(layer_mix=[5]))
