"""Layer mix on the MI355X: mtvaf_layer_mix_fwd / _dots / _inject against the float64 reference and the
derived bounds of layer_mix_cases.py, the exact equalities of the contract, and `TVNetSAModel2` / `TVNetSAModel` with
args.layer_mix against the same model run padded -- where the intermediate hidden states are differentiable without this
feature -- with the mix written in eager torch over ``output_hidden_states``."""
import contextlib
import functools

import pytest
import torch

import layer_mix_cases as LC
import params as P
from test_model_gpu import DEV, LABELS, _prompt_inputs, close, hf_config, make_args
from test_ops_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
OK, ERR_SHAPE, ERR_ARG, ERR_WORKSPACE = 0, -1, -3, -4  # include/mtvaf_hip.h


@functools.lru_cache(maxsize=None)
def _dev_inputs(i):
    states, dy, a, g = LC.make_inputs(i)
    return [h.contiguous().to(DEV) for h in states], dy.to(DEV), a.to(DEV), g.to(DEV)


def _run_kernels(hip, i):
    states, dy, a, g = _dev_inputs(i)
    y = hip.layer_mix_fwd(states, a, g, out=torch.full_like(states[0], float("nan")))
    da, dg, coef = hip.layer_mix_dots(states, dy, a, g)
    return y, da, dg, coef


# ---- 1. the kernels against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=LC.IDS)
def test_kernels_stay_within_four_times_the_eager_chains_error(hip, i):
    """Bound: layer_mix_cases.bounds -- FACTOR x the error of the fp32 eager chain per magnitude class, ULPS ulps where that chain is
    exact.  Measured worst ratios of the kernels' error to the eager chain's over all cases (one MI355X): y 1.60, injected gradients
    2.00, d scalars 1.57, d gamma 1.80 -- the bound is 4; each case prints its own."""
    K, rows, H, _, gamma = LC.CASES[i]
    ref, bound = LC.bounds(i)
    states, dy, a, g = _dev_inputs(i)
    y, da, dg, coef = _run_kernels(hip, i)
    torch.cuda.synchronize()
    r = dict(y=LC.ratio(y, ref["y"], bound["y"]), dscalars=LC.ratio(da, ref["dscalars"], bound["dscalars"]),
             dgamma=LC.ratio(dg, ref["dgamma"], bound["dgamma"]))
    # the K injected gradients, first-write form: coef[j] * dy
    dh = torch.stack([hip.layer_mix_inject(coef, j, dy) for j in range(K)])
    r["dh"] = LC.ratio(dh, ref["dh"], bound["dh"])
    print(f"[layer_mix {LC.IDS[i]}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
          + f"  (x {LC.FACTOR:g} = error / eager chain's error)", flush=True)
    assert all(v <= 1.0 for v in r.values()), r
    assert bool(torch.isfinite(y).all()), "an element of y was not written"
    if gamma == 0.0:  # exact zeros, and d gamma still the reference's
        assert float(y.abs().max()) == 0.0 and float(da.abs().max()) == 0.0 and float(dh.abs().max()) == 0.0
        assert float(ref["dgamma"].abs()) > 0 and r["dgamma"] <= 1.0
    if K == 1:
        assert float(da.abs().max()) == 0.0


@pytest.mark.parametrize("rows,H", [(1, 64), (65, 768), (257, 1024), (1031, 1024)])
def test_inject_is_one_fused_multiply_add(hip, rows, H):
    """dh = fmaf(c, dy, dh): torch.addcmul in float64 -- the product of two fp32 values is exact there -- rounded once.  The first
    write is the correctly rounded product."""
    gen = torch.Generator().manual_seed(rows)
    scale = LC.column_scale(H)
    dy = torch.randn(rows, H, generator=gen) * scale
    dh = torch.randn(rows, H, generator=gen) * scale
    coef = torch.tensor([0.3, -1.7, 0.0, 1e-3, 1.0], dtype=torch.float32)
    for j in range(coef.numel()):
        c = coef[j].double()
        want = torch.addcmul(dh.double(), dy.double(), c.expand_as(dy)).float()
        got = hip.layer_mix_inject(coef.to(DEV), j, dy.to(DEV), dh.clone().to(DEV))
        assert torch.equal(got.cpu(), want), (j, "add into dh")
        first = hip.layer_mix_inject(coef.to(DEV), j, dy.to(DEV))
        assert torch.equal(first.cpu(), (dy.double() * c).float()), (j, "first write")
    buf = dh.clone().to(DEV)
    assert hip.layer_mix_inject(coef.to(DEV), 0, dy.to(DEV), buf).data_ptr() == buf.data_ptr(), "in place"


def test_same_inputs_same_bits(hip):
    for i in (5, 12):
        a, b = _run_kernels(hip, i), _run_kernels(hip, i)
        for x, z, name in zip(a, b, ("y", "dscalars", "dgamma", "coef")):
            assert torch.equal(x, z), (LC.IDS[i], name)


def test_the_last_state_alone_with_gamma_one_is_a_copy(hip):
    states, dy, a, g = _dev_inputs(2)
    one, zero = torch.ones(1, device=DEV), torch.full((1,), -3.5, device=DEV)
    y = hip.layer_mix_fwd(states[-1:], zero, one)
    assert torch.equal(y, states[-1])
    da, dg, coef = hip.layer_mix_dots(states[-1:], dy, zero, one)
    assert float(da[0]) == 0.0 and float(coef[0]) == 1.0
    assert torch.equal(hip.layer_mix_inject(coef, 0, dy), dy)


def test_argument_checks(hip):
    import ctypes
    L = hip.lib()
    x = torch.zeros(4, 64, device=DEV)
    a, g = torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
    ws = torch.empty(hip.LAYER_MIX_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    ptrs = lambda k, p=None: (ctypes.c_void_p * max(k, 1))(*([p if p is not None else x.data_ptr()] * max(k, 1)))
    st = hip._st()
    fwd = lambda K, arr, sc=a.data_ptr(), ga=g.data_ptr(), y=x.data_ptr(), rows=4, H=64: L.mtvaf_layer_mix_fwd(arr, K, sc, ga, y, rows, H, st)
    assert fwd(2, ptrs(2)) == OK
    for K in (0, -1, 33):
        assert fwd(K, ptrs(33)) == ERR_ARG
    assert fwd(2, None) == ERR_ARG and fwd(2, ptrs(2), sc=None) == ERR_ARG and fwd(2, ptrs(2), ga=None) == ERR_ARG
    assert fwd(2, ptrs(2), y=None) == ERR_ARG and fwd(2, ptrs(2), H=62) == ERR_ARG and fwd(2, ptrs(2), rows=0) == ERR_SHAPE
    null_entry = (ctypes.c_void_p * 2)(x.data_ptr(), None)
    assert fwd(2, null_entry) == ERR_ARG
    out3 = [torch.zeros(2, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)]
    dots = lambda K=2, arr=ptrs(2), dy=x.data_ptr(), H=64, w=ws.data_ptr(), wb=ws.numel(), o=out3[0].data_ptr(): L.mtvaf_layer_mix_dots(
        arr, K, dy, a.data_ptr(), g.data_ptr(), 4, H, w, wb, o, out3[1].data_ptr(), out3[2].data_ptr(), st)
    assert dots() == OK
    assert dots(K=33) == ERR_ARG and dots(K=0) == ERR_ARG and dots(dy=None) == ERR_ARG and dots(H=66) == ERR_ARG
    assert dots(w=None) == ERR_ARG and dots(o=None) == ERR_ARG and dots(arr=null_entry) == ERR_ARG
    assert dots(wb=ws.numel() - 1) == ERR_WORKSPACE
    inj = lambda j=0, K=2, c=out3[2].data_ptr(), dy=x.data_ptr(), dh=x.data_ptr(), H=64, acc=1: L.mtvaf_layer_mix_inject(
        c, j, K, dy, dh, 4, H, acc, st)
    assert inj() == OK and inj(acc=0) == OK
    assert inj(j=2) == ERR_ARG and inj(j=-1) == ERR_ARG and inj(K=33) == ERR_ARG and inj(K=0) == ERR_ARG
    assert inj(c=None) == ERR_ARG and inj(dy=None) == ERR_ARG and inj(dh=None) == ERR_ARG and inj(H=30) == ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.layer_mix_fwd([x] * 33, torch.zeros(33, device=DEV), g)
    with pytest.raises(ValueError):
        hip.layer_mix_fwd([x, x], torch.zeros(3, device=DEV), g)


# ---- 2. through the models -------------------------------------------------------------------------------------------------
CFG = P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
# the tiny batch of the existing GPU tests (too few rows to pack: it runs padded in either layout) and a ragged one that packs
# (279 live rows of 512 -> a 384-row image); both hold a one-token and a full-length sentence
TINY = dict(B=3, S=16, lengths=[16, 1, 9])
RAGGED = dict(B=8, S=64, lengths=[64, 1, 30, 50, 10, 64, 20, 40])
Q0 = "bert.encoder.layer.0.attention.self.query.weight"
QKV = [f"bert.encoder.layer.{l}.attention.self.{n}.weight" for l in (0, 1) for n in ("query", "key", "value")]
WATCH = ["fc.weight", "bert.embeddings.word_embeddings.weight"] + QKV


def _tagger(layer_mix=None, train=True, **kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(alpha=0.0, layer_mix=layer_mix, **kw)
    args.bert_config = hf_config(CFG, dropout=0.0)
    torch.manual_seed(11)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    m.dropout.p = m.img_dropout.p = 0.0  # (all dropout probabilities 0: the head's and the prompt generator's nn.Dropout too)
    return m.train() if train else m.eval()


def _set_mix(m, seed=3):
    """Distinct weights and a scale that is not 1, so that no term of the formula drops out."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.layer_mix.scalars.copy_(torch.randn(m.layer_mix.scalars.shape, generator=g).to(DEV))
        m.layer_mix.gamma.fill_(0.7)


def _batch(shape, seed=5, prefix=True):
    ids, mask, tt, labels = P.text_batch(CFG, seed, shape["B"], shape["S"], lengths=shape["lengths"], lo_id=5)
    labels[:, 0] = 9
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
    if prefix:
        feats, aux, _ = _prompt_inputs(seed + 1, shape["B"], 1)
        kw.update(images=feats, aux_imgs=aux)
    return {k: v.to(DEV) for k, v in kw.items()}


def _grads(m, mix=None):
    """mix: the `LayerMix` a reference run has taken out of the model; its gradients are filed under the names they have inside."""
    torch.cuda.synchronize()
    named = list(m.named_parameters()) + ([("layer_mix." + n, p) for n, p in mix.named_parameters()] if mix is not None else [])
    g = {n: p.grad.detach().clone() for n, p in named if p.grad is not None}
    for _, p in named:
        p.grad = None
    return g


@contextlib.contextmanager
def _eager_mix(m):
    """The reference: the SAME model with the option taken off and the padded layout, its encoder's ``last_hidden_state`` replaced
    by the mix written in eager torch over ``output_hidden_states`` (differentiable in a padded run without this feature).  The
    module's own parameters are the leaves, so their gradients land where the fused run's do."""
    from mtvaf_amd import engine
    mix = m.layer_mix

    def hook(mod, inp, out):
        hs = out["hidden_states"]
        s = torch.softmax(mix.scalars, 0)
        out["last_hidden_state"] = mix.gamma * sum(s[j] * hs[k] for j, k in enumerate(mix.layers))
        return out
    m.layer_mix = None
    h = m.bert.register_forward_hook(hook)
    try:
        with engine.padding_free(False):
            yield mix
    finally:
        h.remove()
        m.layer_mix = mix


def _step(m, kw, mix=None, **extra):
    out = m(**kw, **extra)
    out.loss.backward()
    return out.loss.detach().clone(), list(out.logits), _grads(m, mix)


def _assert_matches_reference(got, ref, names=WATCH, mix=True):
    """Bounds of tests/test_configs_gpu.py for the assembled step against its reference: the loss within 1e-3 relative, gradients
    with close(rtol=3e-3) (atol 3e-3 of the largest entry) -- the fused mix and the eager chain differ in rounding only (fmaf
    against multiply-add, one injection per boundary against K gradient tensors added by autograd)."""
    (l1, t1, g1), (l0, t0, g0) = got, ref
    assert abs(float(l1) - float(l0)) <= 1e-3 * abs(float(l0)), (float(l1), float(l0))
    for n in (["layer_mix.scalars", "layer_mix.gamma"] if mix else []) + list(names):
        assert n in g1 and n in g0, n
        close(g1[n], g0[n], rtol=3e-3, name=n)


@pytest.mark.parametrize("layers", ["all", [0, 2], [1]], ids=["all", "first+last", "middle"])
@pytest.mark.parametrize("shape,unpad", [(TINY, False), (RAGGED, False), (RAGGED, True)], ids=["tiny", "ragged-padded", "ragged-packed"])
def test_tagger_matches_the_eager_mix_of_the_padded_run(shape, unpad, layers, f32_arith):
    from mtvaf_amd import engine
    m = _tagger(layer_mix=layers)
    _set_mix(m)
    kw = _batch(shape)
    with engine.padding_free(unpad):
        got = _step(m, kw)
        assert (engine.LAST_PACK is not None) == unpad, "the run did not use the layout the test asked for"
    with _eager_mix(m) as mix:
        ref = _step(m, kw, mix)
    names = WATCH if layers != [1] else [n for n in WATCH if ".layer.1." not in n]  # (nothing reaches the layer above the mix)
    _assert_matches_reference(got, ref, names)
    assert got[1] == ref[1], "decoded tags"
    if layers == [1]:
        assert not any(".layer.1." in n and float(g.abs().max()) > 0 for n, g in got[2].items())


def test_padded_and_padding_free_fused_runs_agree(f32_arith):
    """The criteria of tests/test_unpad_gpu.py (test_unpadded_run_equals_padded_run): the loss within 2e-6 relative, the tags equal,
    gradients close(rtol=2e-5, atol=4e-6 of the largest entry + 1e-9), the word table (float-atomic scatter-add) rtol=1e-4,
    atol=2e-6 of the largest entry.  The mixed state itself: the same bits on live rows, zeros on masked ones."""
    from mtvaf_amd import engine
    m = _tagger(layer_mix="all")
    _set_mix(m)
    kw = _batch(RAGGED)
    res = []
    for unpad in (False, True):
        cap = {}
        h = m.bert.register_forward_hook(lambda mod, inp, out: cap.update(mixed=out.mixed_hidden_state.detach().clone()))
        with engine.padding_free(unpad):
            res.append(_step(m, kw) + (engine.LAST_PACK is not None, cap["mixed"]))
        h.remove()
    (l0, t0, g0, p0, y0), (l1, t1, g1, p1, y1) = res
    assert not p0 and p1, "the second run did not pack"
    valid = kw["attention_mask"].bool()
    assert torch.equal(y1[valid], y0[valid]) and float(y1[~valid].abs().max()) == 0.0
    assert abs(float(l0) - float(l1)) <= 2e-6 * abs(float(l0)), (float(l0), float(l1))
    assert t0 == t1 and set(g0) == set(g1) and {"layer_mix.scalars", "layer_mix.gamma", Q0} <= set(g0)
    for n in g0:
        if "word_embeddings" in n:
            close(g1[n], g0[n], rtol=1e-4, atol=2e-6 * float(g0[n].abs().max()), name=n)
        else:
            close(g1[n], g0[n], rtol=2e-5, atol=4e-6 * float(g0[n].abs().max()) + 1e-9, name=n)


@pytest.mark.parametrize("shape,unpad", [(TINY, False), (RAGGED, True)], ids=["tiny", "ragged-packed"])
def test_gradient_reaches_layer_0_through_the_mix_alone(shape, unpad, f32_arith):
    """layers = [0, 1] on the 2-layer encoder: the last layer is not in the mix, so everything layer 0 and the embeddings receive
    came through the injection below the encoder's top -- the path a padding-free run did not have."""
    from mtvaf_amd import engine
    m = _tagger(layer_mix=[0, 1])
    _set_mix(m)
    kw = _batch(shape)
    with engine.padding_free(unpad):
        got = _step(m, kw)
        assert (engine.LAST_PACK is not None) == unpad
    with _eager_mix(m) as mix:
        ref = _step(m, kw, mix)
    names = [n for n in WATCH if ".layer.1." not in n]
    assert float(got[2][Q0].abs().max()) > 0 and float(got[2]["bert.embeddings.word_embeddings.weight"].abs().max()) > 0
    _assert_matches_reference(got, ref, names)


def test_bf16_compute_mode_runs_the_same_mix():
    """Mixed-precision mode (512 padded rows: the bf16-operand kernels run): the mix reads the fp32 residual-stream states there
    too.  Bounds of that mode in tests/test_unpad_gpu.py: the loss within 5e-3, gradients within 5e-2 in relative norm."""
    from mtvaf_amd import engine, hip as H
    H.set_compute_dtype("bf16")
    try:
        m = _tagger(layer_mix="all")
        _set_mix(m)
        kw = _batch(RAGGED)
        with engine.padding_free(False):
            got = _step(m, kw)
        with _eager_mix(m) as mix:
            ref = _step(m, kw, mix)
        assert abs(float(got[0]) - float(ref[0])) <= 5e-3 * abs(float(ref[0]))
        for n in ["layer_mix.scalars", "layer_mix.gamma"] + WATCH:
            assert torch.isfinite(got[2][n]).all()
            rel = float((got[2][n] - ref[2][n]).norm() / ref[2][n].norm())
            assert rel < 5e-2, (n, rel)
    finally:
        H.set_compute_dtype("fp32")


def test_python_orchestrated_execution_honours_the_mix():
    """engine.NATIVE_EXEC off: the same node on the Python-level kernel sequence."""
    from mtvaf_amd import engine
    m = _tagger(layer_mix="all")
    _set_mix(m)
    kw = _batch(TINY)
    was, engine.NATIVE_EXEC = engine.NATIVE_EXEC, False
    try:
        got = _step(m, kw)
    finally:
        engine.NATIVE_EXEC = was
    with _eager_mix(m) as mix:
        ref = _step(m, kw, mix)
    _assert_matches_reference(got, ref)


def test_last_layer_alone_is_the_model_without_the_option(pad_mode):
    m = _tagger(layer_mix=[-1], train=False)
    plain = _tagger(train=False)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if "layer_mix" not in k})
    kw = _batch(RAGGED)
    cap = {}
    h = m.bert.register_forward_hook(lambda mod, inp, out: cap.update(out=out))
    a = m(**kw)
    h.remove()
    b = plain(**kw)
    assert float(m.layer_mix.gamma.detach()) == 1.0 and m.layer_mix.layers == (2,)
    assert torch.equal(cap["out"].mixed_hidden_state, cap["out"]["last_hidden_state"])
    assert torch.equal(a.loss, b.loss) and list(a.logits) == list(b.logits)


def test_gamma_zero_gives_exact_zeros_and_still_learns_gamma():
    m = _tagger(layer_mix="all")
    _set_mix(m)
    with torch.no_grad():
        m.layer_mix.gamma.zero_()
    kw = _batch(TINY)
    cap = {}
    h = m.bert.register_forward_hook(lambda mod, inp, out: cap.update(mixed=out.mixed_hidden_state.detach()))
    loss, _, g = _step(m, kw)
    h.remove()
    assert float(cap["mixed"].abs().max()) == 0.0 and float(g["layer_mix.scalars"].abs().max()) == 0.0
    assert float(g[Q0].abs().max()) == 0.0 and float(g["layer_mix.gamma"].abs()) > 0
    with _eager_mix(m) as mix:
        ref = _step(m, kw, mix)
    close(g["layer_mix.gamma"], ref[2]["layer_mix.gamma"], rtol=3e-3, name="d gamma at gamma = 0")


def test_word_pooling_reads_the_mixed_state():
    from test_wordpool_gpu import WC
    m = _tagger(layer_mix="all", word_pooling="mean")
    _set_mix(m)
    kw = _batch(RAGGED)
    gen = torch.Generator().manual_seed(5)
    t2w = torch.tensor([WC.sentence(RAGGED["S"], n, WC._random_pieces(gen, n, hi=3)) for n in RAGGED["lengths"]],
                       dtype=torch.int32).to(DEV)
    got = _step(m, kw, token_to_word=t2w)
    with _eager_mix(m) as mix:
        ref = _step(m, kw, mix, token_to_word=t2w)
    _assert_matches_reference(got, ref)
    assert got[1] == ref[1]


def test_predict_reads_the_mixed_state():
    m = _tagger(layer_mix="all", train=False)
    _set_mix(m)
    kw = _batch(RAGGED)
    args3 = (kw["input_ids"], kw["attention_mask"], kw["token_type_ids"])
    got = m.predict(*args3, images=kw["images"], aux_imgs=kw["aux_imgs"])
    with _eager_mix(m):
        want = m.predict(*args3, images=kw["images"], aux_imgs=kw["aux_imgs"])
    torch.cuda.synchronize()
    assert torch.equal(got["tags"], want["tags"])
    with torch.no_grad():
        m.layer_mix.scalars.copy_(torch.tensor([9.0, 0.0, -9.0], device=DEV))  # (now nearly the embedding output alone)
    moved = m.predict(*args3, images=kw["images"], aux_imgs=kw["aux_imgs"])
    torch.cuda.synchronize()
    assert not torch.equal(moved["tags"], got["tags"]), "predict does not read the mix"


# ---- the span model ----------------------------------------------------------------------------------------------------------
def _span_model(layer_mix):
    from mtvaf_amd.models.bert_model import TVNetSAModel
    args = make_args(use_prefix=False, gcn_layer_number=0, num_layers=0, aug_type="span_cutoff", aug_cutoff_ratio=0.3,
                     aug_ce_loss=1.0, aug_js_loss=1.0, layer_mix=layer_mix)
    args.bert_config = hf_config(CFG, dropout=0.0)
    torch.manual_seed(0)
    m = TVNetSAModel(LABELS, None, args).to(DEV)
    m.dropout.p = 0.0
    return m.train()


def _span_batch(B=6, S=32, M=5):
    lengths = [S, 20, 1, 31, 14, 26][:B]
    ids, mask, tt, _ = P.text_batch(CFG, 3, B, S, lengths, lo_id=5)
    starts, ends, spos, epos, pol, lm = P.span_batch(CFG, 4, B, S, M, [max(n, 2) for n in lengths])
    batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, start_positions=spos, end_positions=epos,
                 span_starts=starts, span_ends=ends, polarity_labels=pol, label_masks=lm)
    return {k: v.to(DEV) for k, v in batch.items()}


def test_span_model_matches_the_eager_mix_and_the_cutoff_step_runs():
    m = _span_model("all")
    _set_mix(m)
    batch = _span_batch()
    out = m(**batch)
    out.loss.backward()
    got = (out.loss.detach().clone(), None, _grads(m))
    with _eager_mix(m) as mix:
        out = m(**batch)
        out.loss.backward()
        ref = (out.loss.detach().clone(), None, _grads(m, mix))
    names = ["binary_affine.weight", "classifier.weight", "bert.embeddings.word_embeddings.weight"] + QKV
    _assert_matches_reference(got, ref, names)
    # the two-pass cutoff step: both passes read the mix; finite gradients for both parameters
    out = m.forward_with_cutoff(**batch)
    out.loss.backward()
    g = _grads(m)
    assert torch.isfinite(out.loss) and Q0 in g
    for n in ("layer_mix.scalars", "layer_mix.gamma"):
        assert torch.isfinite(g[n]).all() and float(g[n].abs().max()) > 0, n


# ---- the captured step -------------------------------------------------------------------------------------------------------
def test_graph_replays_equal_eager_steps_with_the_mix_parameters_in_the_optimizer():
    from mtvaf_amd import engine
    from mtvaf_amd.graph import GraphedTrainStep
    from mtvaf_amd.optim import AdamW, ScheduleMirror, finetune_param_groups, linear_warmup_factor, schedule_table
    from test_device_schedule_gpu import _distinct_ids, _equal
    factor, betas = linear_warmup_factor(1.0, 20), (0.9, 0.999)
    shape = dict(B=2, S=64, lengths=[64, 37])
    models = []
    for _ in range(2):
        m = _tagger(layer_mix="all", train=False)
        _set_mix(m)
        models.append(m)
    m1, m2 = models
    batch = _distinct_ids(_batch(shape), CFG)
    groups = lambda m: finetune_param_groups(m, 1e-3, layer_lr_decay=0.9)
    o1 = AdamW(groups(m1), model=m1, device_schedule=schedule_table(factor, 4, betas))
    o2 = AdamW(groups(m2), model=m2, device_schedule=schedule_table(factor, 4, betas))
    s1, s2 = ScheduleMirror(o1), ScheduleMirror(o2)
    g = GraphedTrainStep(m2, batch, optimizer=o2)
    try:
        for _ in range(3):
            with engine.padding_free(False):
                m1(**batch).loss.backward()
            o1.step()
            s1.step()
            o1.zero_grad(set_to_none=True)
            g(**batch)
            s2.step()
            o2.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        start = _tagger(layer_mix="all", train=False)
        _set_mix(start)
        for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
            assert _equal(p, q), n
        for n in ("layer_mix.scalars", "layer_mix.gamma", "fc.weight", Q0):
            assert not _equal(dict(m2.named_parameters())[n], dict(start.named_parameters())[n]), f"{n} did not train"
    finally:
        g.close()


# ---- the default ---------------------------------------------------------------------------------------------------------------
def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if "cuda" in str(e.device_type).lower()}


def test_without_the_option_nothing_is_added_and_nothing_is_launched():
    plain, on = _tagger(), _tagger(layer_mix="all")
    assert plain.layer_mix is None and not any("layer_mix" in k for k in plain.state_dict())
    assert set(on.state_dict()) - set(plain.state_dict()) == {"layer_mix.scalars", "layer_mix.gamma"}
    kw = _batch(RAGGED)
    _step(plain, kw)  # (first-call allocations and lazily built tables out of the profile)
    _step(on, kw)
    names_on = _kernel_names(lambda: _step(on, kw))
    names_off = _kernel_names(lambda: _step(plain, kw))
    mix_on = sorted(n for n in names_on if "layer_mix" in n)
    assert len(mix_on) >= 4, f"the profiler did not see the mix's kernels of the step with the option on: {mix_on}"
    assert names_off and not [n for n in names_off if "layer_mix" in n]
    out = plain.bert(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], token_type_ids=kw["token_type_ids"])
    assert not hasattr(out, "mixed_hidden_state")
