"""Per-sentence CRF likelihoods (mtvaf_crf_llh_fwd / _bwd), tag marginals (mtvaf_crf_marginals) and the layers above
them -- CRF.forward(reduction='none' | 'token_mean'), CRF.marginals, TVNetSAModel2's crf_reduction /
output_tag_marginals -- on the MI355X, against the float64 oracle under the acceptance rule of crf_llh_cases."""
import types

import pytest
import torch
from transformers import BertConfig

import crf_llh_cases as L
import params as P
from oracle import mtvaf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def _dev(inputs):
    return tuple(t.to(DEV) for t in inputs)


def _on(mask):
    on = mask.bool().clone()
    on[:, 0] = True
    return on


# ---- 1. C ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES, ids=str)
def test_llh_fwd_bwd_abi(hip, case):
    """llh [B]; then the backward with per-sentence weights of mixed sign (one an exact 0) accumulated onto prefilled
    parameter gradients: d(emissions) exactly zero at masked steps and for the zero-weight sentence."""
    ref = L.reference(case)
    B, S, C = ref.inputs[0].shape
    em, tags, mask, start, end, trans = _dev(ref.inputs)
    ws, wsb = hip.crf_workspace(B, S, C, DEV)
    llh = torch.full((B,), 7.0, device=DEV)
    hip.crf_llh_fwd(em, tags, mask, start, end, trans, llh, ws, wsb)
    L.check(ref, "llh", llh)
    dem = torch.full((B, S, C), 7.0, device=DEV)
    ds, de, dt = torch.full((C,), 0.5, device=DEV), torch.full((C,), -2.0, device=DEV), torch.full((C, C), 3.0, device=DEV)
    hip.crf_llh_bwd(ref.w.to(DEV), em, tags, mask, start, end, trans, dem, ds, de, dt, True, ws, wsb)
    L.check(ref, "dem", dem)
    L.check(ref, "dstart", ds, add=0.5)
    L.check(ref, "dend", de, add=-2.0)
    L.check(ref, "dtrans", dt, add=3.0)
    dem = dem.cpu()
    assert bool((dem[~_on(ref.inputs[2])] == 0).all())
    if B >= 2:
        assert float(ref.w[1]) == 0.0 and bool((dem[1] == 0).all())
    # accumulate = 0 overwrites
    ds2, de2, dt2 = torch.full((C,), 9.0, device=DEV), torch.full((C,), 9.0, device=DEV), torch.full((C, C), 9.0, device=DEV)
    hip.crf_llh_bwd(ref.w.to(DEV), em, tags, mask, start, end, trans, torch.empty_like(em), ds2, de2, dt2, False, ws, wsb)
    L.check(ref, "dstart", ds2)
    L.check(ref, "dend", de2)
    L.check(ref, "dtrans", dt2)


# ---- 2. marginals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES, ids=str)
def test_marginals_abi(hip, case):
    ref = L.reference(case)
    B, S, C = ref.inputs[0].shape
    em, _, mask, start, end, trans = _dev(ref.inputs)
    ws, wsb = hip.crf_workspace(B, S, C, DEV)
    marg, logz = torch.full((B, S, C), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    hip.crf_marginals(em, mask, start, end, trans, marg, logz, ws, wsb)
    L.check(ref, "marg", marg)
    L.check(ref, "logz", logz)
    m, on = marg.cpu(), _on(ref.inputs[2])
    assert bool((m[~on] == 0).all())
    assert float(m.min()) >= 0.0
    assert float((m.sum(-1)[on].double() - 1).abs().max()) <= ref.bound["marg"]
    marg2 = torch.full((B, S, C), 7.0, device=DEV)
    hip.crf_marginals(em, mask, start, end, trans, marg2, None, ws, wsb)  # logz is optional
    assert torch.equal(marg2, marg)


@pytest.mark.parametrize("S,C", [(8, 65), (513, 17)])
def test_new_entry_points_reject_unsupported_shapes(hip, S, C):
    """The same error as mtvaf_crf_nll_* for the same bad shapes, before any launch."""
    B = 2
    em = torch.randn(B, S, C, device=DEV)
    tags = torch.zeros(B, S, dtype=torch.long, device=DEV)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    start, end, trans = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, C, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    llh, w = torch.full((B,), 7.0, device=DEV), torch.ones(B, device=DEV)
    dem = torch.full((B, S, C), 7.0, device=DEV)
    with pytest.raises(Exception):
        hip.crf_llh_fwd(em, tags, mask, start, end, trans, llh, ws, ws.numel())
    with pytest.raises(Exception):
        hip.crf_llh_bwd(w, em, tags, mask, start, end, trans, dem, start, end, trans, False, ws, ws.numel())
    with pytest.raises(Exception):
        hip.crf_marginals(em, mask, start, end, trans, dem, llh, ws, ws.numel())
    torch.cuda.synchronize()
    assert bool((llh == 7).all()) and bool((dem == 7).all()) and int(ws.sum()) == 0


# ---- 3. brute-force known answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.BRUTE, ids=str)
def test_bruteforce_known_answers(hip, case):
    ref = L.brute_reference(case)
    B, S, C = ref.inputs[0].shape
    em, tags, mask, start, end, trans = _dev(ref.inputs)
    ws, wsb = hip.crf_workspace(B, S, C, DEV)
    llh = torch.empty(B, device=DEV)
    hip.crf_llh_fwd(em, tags, mask, start, end, trans, llh, ws, wsb)
    marg, logz = torch.empty(B, S, C, device=DEV), torch.empty(B, device=DEV)
    hip.crf_marginals(em, mask, start, end, trans, marg, logz, ws, wsb)
    for name, got in (("llh", llh), ("logz", logz), ("marg", marg)):
        assert L.ratio(name, got, ref.brute[name], ref.bound[name]) <= 1.0, name


# ---- 4. module -------------------------------------------------------------------------------------------------------
MODULE_CASES = [(3, 17, 11, 1), (4, 66, 48, -1)]


def _module(case, batch_first=True):
    from mtvaf_amd.modules.crf import CRF
    ref = L.reference(case)
    em, tags, mask, start, end, trans = ref.inputs
    crf = CRF(em.shape[2], batch_first=batch_first).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start)
        crf.end_transitions.copy_(end)
        crf.transitions.copy_(trans)
    emg, tg, mk = em.to(DEV).requires_grad_(True), tags.to(DEV), mask.to(DEV)
    if not batch_first:
        emg = em.transpose(0, 1).contiguous().to(DEV).requires_grad_(True)
        tg, mk = tg.transpose(0, 1).contiguous(), mk.transpose(0, 1).contiguous()
    return ref, crf, emg, tg, mk


@pytest.mark.parametrize("case", MODULE_CASES, ids=str)
@pytest.mark.parametrize("batch_first", [True, False])
def test_module_weighted_none_backward(case, batch_first):
    ref, crf, em, tags, mask = _module(case, batch_first)
    llh = crf(em, tags, mask=mask, reduction="none")
    assert tuple(llh.shape) == (ref.inputs[0].shape[0],)
    L.check(ref, "llh", llh)
    (ref.w.to(DEV) * llh).sum().backward()
    L.check(ref, "dem", em.grad if batch_first else em.grad.transpose(0, 1))
    L.check(ref, "dstart", crf.start_transitions.grad)
    L.check(ref, "dend", crf.end_transitions.grad)
    L.check(ref, "dtrans", crf.transitions.grad)


@pytest.mark.parametrize("case", MODULE_CASES, ids=str)
def test_module_reductions_agree_and_token_mean(case):
    ref, crf, em, tags, mask = _module(case)
    B = em.shape[0]
    none = crf(em, tags, mask=mask, reduction="none").detach().double().cpu()
    mean, total = (float(crf(em, tags, mask=mask, reduction=r)) for r in ("mean", "sum"))
    llh64, llh32 = ref.r64["llh"], ref.r32["llh"]
    for name, got_none, got, r64, r32 in (("mean", float(none.mean()), mean, llh64.mean(), llh32.mean()),
                                          ("sum", float(none.sum()), total, llh64.sum(), llh32.sum())):
        bnd = L.bound("llh", r64.reshape(1), r32.reshape(1))
        assert abs(got_none - float(r64)) <= bnd and abs(got - float(r64)) <= bnd and abs(got_none - got) <= bnd, name
    # token_mean: value and gradients against the oracle
    inputs = ref.inputs
    for dtype in (torch.float64, torch.float32):
        e_, s_, n_, t_ = (x.to(dtype).clone().requires_grad_(True) for x in (inputs[0], inputs[3], inputs[4], inputs[5]))
        v = O.crf_log_likelihood(e_, inputs[1], inputs[2], s_, n_, t_, "token_mean")
        g = torch.autograd.grad(v, [e_, s_, n_, t_])
        if dtype == torch.float64:
            v64, g64 = v.detach(), g
        else:
            v32, g32 = v.detach(), g
    tm = crf(em, tags, mask=mask, reduction="token_mean")
    assert tm.dim() == 0
    assert L.ratio("llh", tm, v64, L.bound("llh", v64.reshape(1), v32.reshape(1))) <= 1.0
    tm.backward()
    for name, got, a, b in zip(("dem", "dstart", "dend", "dtrans"),
                               (em.grad, crf.start_transitions.grad, crf.end_transitions.grad, crf.transitions.grad), g64, g32):
        assert L.ratio(name, got, a, L.bound(name, a, b)) <= 1.0, name


def test_module_marginals_and_invalid_reduction():
    ref, crf, em, tags, mask = _module(MODULE_CASES[1])
    marg, logz = crf.marginals(em, mask, return_logz=True)
    assert not marg.requires_grad and not logz.requires_grad and marg.grad_fn is None
    assert tuple(marg.shape) == tuple(em.shape) and tuple(logz.shape) == (em.shape[0],)
    L.check(ref, "marg", marg)
    L.check(ref, "logz", logz)
    assert torch.equal(crf.marginals(em, mask), marg)
    ref2, crf2, em2, tags2, mask2 = _module(MODULE_CASES[1], batch_first=False)
    m2 = crf2.marginals(em2, mask2)
    assert tuple(m2.shape) == tuple(em2.shape) and torch.equal(m2.transpose(0, 1), marg)
    nomask = crf.marginals(em)  # mask = None: every step counts
    assert float((nomask.sum(-1) - 1).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        crf(em, tags, mask=mask, reduction="batch_mean")


@pytest.mark.parametrize("case", MODULE_CASES, ids=str)
def test_mean_bits_unchanged_by_none_and_marginals_calls(case):
    _, crf, em, tags, mask = _module(case)
    params = [em, crf.start_transitions, crf.end_transitions, crf.transitions]

    def mean():
        v = crf(em, tags, mask=mask, reduction="mean")
        return [v.detach().clone()] + [g.clone() for g in torch.autograd.grad(v, params)]
    before = mean()
    llh = crf(em, tags, mask=mask, reduction="none")
    torch.autograd.grad(llh.sum(), params)
    crf.marginals(em, mask)
    for a, b in zip(before, mean()):
        assert torch.equal(a, b)


# ---- 5. model --------------------------------------------------------------------------------------------------------
LABELS10 = ["O", "B-NEU", "I-NEU", "B-POS", "I-POS", "B-NEG", "I-NEG", "X", "[CLS]", "[SEP]"]
CFG = P.EncCfg(vocab_size=200, hidden=128, heads=2, inter=256, layers=2, max_pos=64)


def _tvnet2(**kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    hf = BertConfig(vocab_size=CFG.vocab_size, hidden_size=CFG.hidden, num_hidden_layers=CFG.layers,
                    num_attention_heads=CFG.heads, intermediate_size=CFG.inter, max_position_embeddings=CFG.max_pos,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", bert_config=hf, use_prefix=False, vao=False, noauxloss=True,
                                 use_probe=False, n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768, device=DEV,
                                 resnet_root=None, use_152=False, **kw)
    m = TVNetSAModel2(LABELS10, None, args)
    sd = {**{"bert." + k: v for k, v in P.encoder_params(CFG, 1).items()}, **P.head_params(CFG, 2)}
    assert not m.load_state_dict(sd, strict=False)[1]
    return m.to(DEV).eval()


def test_model_tag_marginals_and_crf_reduction():
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(CFG, 3, 3, 16, lengths=[16, 9, 5]))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
    plain = _tvnet2()
    out0 = plain(**kw)
    assert plain.last_tag_marginals is None
    m = _tvnet2(output_tag_marginals=True)  # crf_reduction left out: today's nll_mean call
    out1 = m(**kw)
    assert torch.equal(out1.loss, out0.loss)
    mask_u8 = mask.to(torch.uint8)
    # the same emissions, recomputed (eval mode: no dropout; the head runs the linear kernel on fc's parameters)
    from mtvaf_amd import engine
    hs = m.bert(input_ids=ids, attention_mask=mask, token_type_ids=tt, output_hidden_states=True)["last_hidden_state"]
    em = engine.LinearFunction.apply(hs, m.fc.weight, m.fc.bias, False).detach()
    marg = m.last_tag_marginals
    assert tuple(marg.shape) == (3, 16, m.num_labels) and not marg.requires_grad
    assert torch.equal(marg, m.crf.marginals(em, mask_u8))
    assert bool((marg[~mask.bool()] == 0).all()) and float((marg.sum(-1)[mask.bool()] - 1).abs().max()) <= 1e-4
    m.args.output_tag_marginals = False
    m(**kw)
    assert m.last_tag_marginals is None
    # crf_reduction: the loss is -llh reduced
    emc, lab, mk = em.cpu(), labels.cpu(), mask_u8.cpu()
    start, end, trans = (p.detach().cpu() for p in (m.crf.start_transitions, m.crf.end_transitions, m.crf.transitions))
    for red in ("token_mean", "sum", "mean"):
        m.args.crf_reduction = red
        loss = m(**kw).loss
        want = [-O.crf_log_likelihood(emc.to(dt), lab, mk, start.to(dt), end.to(dt), trans.to(dt), red)
                for dt in (torch.float64, torch.float32)]
        assert L.ratio("llh", loss, want[0], L.bound("llh", want[0].reshape(1), want[1].reshape(1))) <= 1.0, red
        if red == "mean":
            assert torch.equal(loss, out0.loss)
    m.args.crf_reduction = "token_mean"
    m.zero_grad(set_to_none=True)
    m(**kw).loss.backward()
    assert m.crf.transitions.grad is not None and bool(torch.isfinite(m.fc.weight.grad).all())


# ---- 6. graph capture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MODULE_CASES, ids=str)
def test_graph_capture_of_none_forward_backward_and_marginals(case):
    ref, crf, em, tags, mask = _module(case)
    w = ref.w.to(DEV)
    params = [em, crf.start_transitions, crf.end_transitions, crf.transitions]

    def step():
        llh = crf(em, tags, mask=mask, reduction="none")
        grads = torch.autograd.grad((w * llh).sum(), params)
        return [llh.detach(), *grads, *crf.marginals(em, mask, return_logz=True)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.fill_(7.0)  # (what the capture's dry pass left is not the result)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
