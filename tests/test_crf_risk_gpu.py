"""The expected-cost (risk) entry points (mtvaf_crf_risk_{fwd,bwd}) and the layers above them -- engine.CRFRiskFunction /
CRFMarginalsFunction, CRF.expected_cost / hamming_risk / differentiable_marginals, TVNetSAModel2's args.crf_risk_weight -- on the
MI355X, against the float64 references under the acceptance rule of crf_risk_cases.

Largest err / bound per quantity over this file, one run on one MI355X: risk 0.008, logz 0.004, marg
0.003, dem 0.006, dstart 0.021, dend 0.017, dtrans 0.010, dcost 0.003."""
import pytest
import torch

import crf_lattice_cases as X
import crf_risk_cases as R
import params as P
from test_crf_lattice_gpu import tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRADS = ("dem", "dcost", "dstart", "dend", "dtrans")


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _run(hip, inp, cost, w, accumulate=False, fill=(0.0, 0.0, 0.0)):
    em, _, mask, start, end, trans = _dev(*inp)
    cost, w = _dev(cost, w)
    B, S, C = em.shape
    ws, wsb = hip.crf_risk_workspace(B, S, C, DEV)
    risk, logz, marg = torch.full((B,), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV), torch.full((B, S, C), 7.0, device=DEV)
    hip.crf_risk_fwd(em, cost, mask, start, end, trans, risk, logz, marg, ws, wsb)
    dem, dcost = torch.full((B, S, C), 7.0, device=DEV), torch.full((B, S, C), 7.0, device=DEV)
    ds, de, dt = torch.full((C,), fill[0], device=DEV), torch.full((C,), fill[1], device=DEV), torch.full((C, C), fill[2], device=DEV)
    hip.crf_risk_bwd(w, em, cost, mask, start, end, trans, dem, dcost, ds, de, dt, accumulate, ws, wsb)
    return dict(risk=risk, logz=logz, marg=marg, dem=dem, dcost=dcost, dstart=ds, dend=de, dtrans=dt)


def _crf(C, start, end, trans, batch_first=True):
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(C, batch_first=batch_first).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start), crf.end_transitions.copy_(end), crf.transitions.copy_(trans)
    return crf


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["h", "r"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_fwd_bwd_abi(hip, shape, pattern):
    ref = R.reference(shape, pattern)
    B = shape[0]
    got = _run(hip, ref.inputs, ref.cost, ref.w)
    for name in R.QUANTITIES:
        R.check(ref, name, got[name])
    on = R.live(ref.inputs[2])
    dem, dcost, marg = got["dem"].cpu(), got["dcost"].cpu(), got["marg"].cpu()
    assert bool((dem[~on] == 0).all()) and bool((dcost[~on] == 0).all()) and bool((marg[~on] == 0).all())
    if B >= 2:
        assert float(ref.w[1]) == 0.0 and bool((dem[1] == 0).all()) and bool((dcost[1] == 0).all())
    colsum = float(dem.double().sum(-1)[on].abs().max())
    print(f"crf-risk column sum of dem {colsum:.3e} (bound {ref.bound['dem']:.3e})")
    assert colsum <= ref.bound["dem"]
    again = _run(hip, ref.inputs, ref.cost, ref.w)
    for name in got:
        assert torch.equal(got[name], again[name]), name


def test_accumulate_and_optional_outputs(hip):
    ref = R.reference((3, 17, 11, 1), "r")
    got = _run(hip, ref.inputs, ref.cost, ref.w, accumulate=True, fill=(0.5, -2.0, 3.0))
    R.check(ref, "dstart", got["dstart"], add=0.5)
    R.check(ref, "dend", got["dend"], add=-2.0)
    R.check(ref, "dtrans", got["dtrans"], add=3.0)
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    cost, w = _dev(ref.cost, ref.w)
    ws, wsb = hip.crf_risk_workspace(3, 17, 11, DEV)
    risk, dem = torch.empty(3, device=DEV), torch.empty(3, 17, 11, device=DEV)
    ds, de, dt = torch.empty(11, device=DEV), torch.empty(11, device=DEV), torch.empty(11, 11, device=DEV)
    hip.crf_risk_fwd(em, cost, mask, start, end, trans, risk, None, None, ws, wsb)  # logz, marg and dcost are optional
    hip.crf_risk_bwd(w, em, cost, mask, start, end, trans, dem, None, ds, de, dt, False, ws, wsb)
    plain = _run(hip, ref.inputs, ref.cost, ref.w)
    assert torch.equal(risk, plain["risk"]) and torch.equal(dem, plain["dem"]) and torch.equal(dt, plain["dtrans"])


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_zero_cost_constant_shift_and_masked_nan(hip, shape):
    ref = R.reference(shape, "r")
    got = _run(hip, ref.inputs, ref.cost, ref.w)
    # (z) nothing is paid and nothing moves, exactly
    zero = _run(hip, ref.inputs, torch.zeros_like(ref.cost), ref.w)
    for name in ("risk", "dem", "dstart", "dend", "dtrans"):  # (+0.0, also under the negative and the zero weights)
        assert bool((zero[name] == 0).all()) and not bool(torch.signbit(zero[name]).any()), name
    # (k) a per-column constant: the same gradients, the risk moved by the constants' sum over the live columns
    k = R.reference(shape, "k")
    gk = _run(hip, k.inputs, k.cost, k.w)
    for name in GRADS:
        R.check(k, name, gk[name])
    shift = ((k.cost.double() - ref.cost.double())[..., 0] * R.live(ref.inputs[2])).sum(1)
    moved = (gk["risk"].double().cpu() - got["risk"].double().cpu() - shift).abs().max()
    assert float(moved) <= k.bound["risk"] + ref.bound["risk"]
    # (n) NaN at the masked columns is never read
    nan = _run(hip, ref.inputs, R.make_cost(shape, "n", ref.inputs), ref.w)
    for name in got:
        assert bool(torch.isfinite(nan[name]).all()) and torch.equal(nan[name], got[name]), name


@pytest.mark.parametrize("S,C", [(8, 65), (513, 17)])
def test_rejected_shapes_launch_nothing(hip, S, C):
    B = 2
    lib = hip.lib()
    em = torch.randn(B, S, C, device=DEV)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    start, end, trans = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, C, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out, dem = torch.full((B,), 7.0, device=DEV), torch.full((B, S, C), 7.0, device=DEV)
    p, st = hip._p, hip._st()
    assert lib.mtvaf_crf_risk_workspace_bytes(B, S, C) == 0
    assert lib.mtvaf_crf_risk_fwd(p(em), p(em), p(mask), p(start), p(end), p(trans), p(out), None, p(dem), B, S, C, p(ws),
                                  ws.numel(), st) == -1
    assert lib.mtvaf_crf_risk_bwd(p(out), p(em), p(em), p(mask), p(start), p(end), p(trans), p(dem), None, p(start), p(end),
                                  p(trans), 0, B, S, C, p(ws), ws.numel(), st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((dem == 7).all()) and int(ws.sum()) == 0


def test_small_workspace_is_refused(hip):
    ref = R.reference((3, 17, 11, 1), "r")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    ws, wsb = hip.crf_risk_workspace(3, 17, 11, DEV)
    risk, dem = torch.full((3,), 7.0, device=DEV), torch.full((3, 17, 11), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="mtvaf_crf_risk_fwd failed: workspace too small"):
        hip.crf_risk_fwd(em, ref.cost.to(DEV), mask, start, end, trans, risk, None, None, ws, wsb - 4)
    with pytest.raises(RuntimeError, match="mtvaf_crf_risk_bwd failed: workspace too small"):
        hip.crf_risk_bwd(ref.w.to(DEV), em, ref.cost.to(DEV), mask, start, end, trans, dem, None, start.clone(), end.clone(),
                         trans.clone(), False, ws, wsb - 4)
    torch.cuda.synchronize()
    assert bool((risk == 7).all()) and bool((dem == 7).all())


# ---- 2. autograd and the module ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (3, 65, 17, 1)], ids=str)
def test_differentiable_marginals(shape):
    """Forward: CRF.marginals() bit for bit.  Backward with a random cotangent V: the float64 double backward, i.e. the gradient
    of sum_b R_b at cost = V, within that case's dem / dstart / dend / dtrans bounds."""
    inp = X.inputs(shape)
    V = torch.randn(inp[0].shape, generator=torch.Generator().manual_seed(5))
    ref = R.make_reference(inp, V, w=torch.ones(shape[0]))
    em, _, mask, start, end, trans = _dev(*inp)
    crf = _crf(shape[2], start, end, trans)
    e = em.clone().requires_grad_(True)
    marg = crf.differentiable_marginals(e, mask)
    assert marg.requires_grad and torch.equal(marg.detach(), crf.marginals(em, mask))
    marg.backward(V.to(DEV))
    R.check(ref, "dem", e.grad)
    R.check(ref, "dstart", crf.start_transitions.grad)
    R.check(ref, "dend", crf.end_transitions.grad)
    R.check(ref, "dtrans", crf.transitions.grad)


def test_expected_cost_and_hamming_risk_autograd():
    shape = (3, 17, 11, 1)
    ref, href = R.reference(shape, "r"), R.reference(shape, "h")
    em, tags, mask, start, end, trans = _dev(*ref.inputs)
    cost, w = _dev(ref.cost, ref.w)
    n = float(mask.sum())
    for batch_first in (True, False):
        crf = _crf(11, start, end, trans, batch_first)
        lay = (lambda x: x) if batch_first else (lambda x: x.transpose(0, 1))
        e, c = lay(em).clone().requires_grad_(True), lay(cost).clone().requires_grad_(True)
        risk = crf.expected_cost(e, c, lay(mask))
        R.check(ref, "risk", risk)
        (risk * w).sum().backward()
        R.check(ref, "dem", lay(e.grad))
        R.check(ref, "dcost", lay(c.grad))
        R.check(ref, "dstart", crf.start_transitions.grad)
        R.check(ref, "dend", crf.end_transitions.grad)
        R.check(ref, "dtrans", crf.transitions.grad)
        r64 = ref.r64["risk"]
        for red, want, scale in (("sum", r64.sum(), 3.0), ("mean", r64.mean(), 1.0), ("token_mean", r64.sum() / n, 1.0)):
            got = float(crf.expected_cost(lay(em), lay(cost), lay(mask), reduction=red).detach())
            assert abs(got - float(want)) <= ref.bound["risk"] * scale, red
        # the expected number of wrong tags, its rate, and columns dropped by keep
        R.check(href, "risk", crf.hamming_risk(lay(em), lay(tags), lay(mask), reduction="none"))
        rate = float(crf.hamming_risk(lay(em), lay(tags), lay(mask)).detach())
        assert abs(rate - float(href.r64["risk"].sum()) / n) <= href.bound["risk"]
        keep = torch.rand(3, 17, generator=torch.Generator().manual_seed(9)) < 0.6
        keep[:, 0] = False
        kept = keep & R.live(ref.inputs[2])
        wrong = ((1 - href.r64["marg"].gather(2, ref.inputs[1][..., None])[..., 0]) * kept).sum(1)
        got = crf.hamming_risk(lay(em), lay(tags), lay(mask), keep=lay(keep.to(DEV)), reduction="none")
        assert float((got.detach().double().cpu() - wrong).abs().max()) <= href.bound["risk"]
        got = float(crf.hamming_risk(lay(em), lay(tags), lay(mask), keep=lay(keep.to(DEV))).detach())
        assert abs(got - float(wrong.sum()) / float(kept.sum())) <= href.bound["risk"]
        none = lay(torch.zeros(3, 17, dtype=torch.bool, device=DEV))  # nothing counts: the rate is 0, not 0 / 0
        assert float(crf.hamming_risk(lay(em), lay(tags), lay(mask), keep=none).detach()) == 0.0
    e = em.clone().requires_grad_(True)  # a cost that asks for no gradient gets none
    crf.expected_cost(lay(e), lay(cost), lay(mask), reduction="sum").backward()
    assert e.grad is not None and cost.grad is None


# ---- 3. the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unpad", [False, True], ids=["padded", "padding-free"])
@pytest.mark.parametrize("reduction", ["mean", "token_mean"])
def test_model_crf_risk_weight(unpad, reduction):
    from mtvaf_amd import engine
    cfg, m = tiny_model(crf_reduction=reduction)
    B, S = 6, 32
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
    seen = {}
    linear = engine.LinearFunction.apply

    def spy(x, weight, *rest):  # the head's input and output
        y = linear(x, weight, *rest)
        if weight is m.fc.weight:
            seen["h"], seen["em"] = x.detach(), y.detach()
        return y

    def step(weight):
        m.args.crf_risk_weight = weight
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        out = m.train()(**kw)
        out.loss.backward()
        return out.loss.detach().clone(), m.fc.weight.grad.detach().clone()

    was = engine.UNPAD
    engine.UNPAD = unpad
    engine.LinearFunction.apply = spy
    try:
        assert not hasattr(m.args, "crf_risk_weight")
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        out = m.train()(**kw)
        out.loss.backward()
        loss_p, g_p = out.loss.detach().clone(), m.fc.weight.grad.detach().clone()  # the parent's path: no such argument
        assert m.last_crf_risk is None
        loss_0, g_0 = step(0.0)
        assert torch.equal(loss_0, loss_p) and torch.equal(g_0, g_p) and m.last_crf_risk is None
        loss_r, g_r = step(0.5)
    finally:
        del engine.LinearFunction.apply  # (back to the inherited classmethod)
        engine.UNPAD = was
    # float64 reference of the token-mean Hamming risk on the model's own emissions
    em, h = seen["em"].float().cpu(), seen["h"].double().cpu()
    crf = m.crf
    inp = (em, labels.cpu(), mask.cpu().to(torch.uint8), crf.start_transitions.detach().cpu(), crf.end_transitions.detach().cpu(),
           crf.transitions.detach().cpu())
    C = em.shape[2]
    cost = (1.0 - torch.nn.functional.one_hot(labels.cpu(), C).float()) * mask.cpu()[..., None]
    n = float(mask.sum())
    ref = R.make_reference(inp, cost, w=torch.full((B,), 1.0 / n))
    want = float(ref.r64["risk"].sum())  # (the weights 1 / n are in the gradients only)  -> rate below
    rate = want / n
    assert m.last_crf_risk is not None and m.last_crf_risk.is_cuda and not m.last_crf_risk.requires_grad
    bnd = ref.bound["risk"] * B / n
    print(f"crf-risk model rate {float(m.last_crf_risk):.6f} vs {rate:.6f}; loss {float(loss_r):.6f} = {float(loss_0):.6f} + half of it")
    assert abs(float(m.last_crf_risk) - rate) <= bnd
    # loss_0 and loss_r share the seed and the likelihood term bit for bit; loss_r is ONE float32 of their sum, so beside the
    # risk bound there is only that number's own rounding, one ulp = 2^-23 |loss_r|
    ulp = 2.0 ** -23
    assert abs(float(loss_r) - (float(loss_0) + 0.5 * rate)) <= bnd + ulp * abs(float(loss_r))
    # the gradient moves by the chain rule's amount: 3e-3 max-norm relative to THAT amount (not to the whole gradient, which
    # the likelihood dominates), plus one ulp of each of the two float32 gradients whose difference is taken
    delta = 0.5 * torch.einsum("bsc,bsh->ch", ref.r64["dem"], h)
    moved = (g_r - g_0).double().cpu()
    err, size = float((moved - delta).abs().max()), float(delta.abs().max())
    tol = 3e-3 * size + 2 * ulp * float(g_r.abs().max())
    print(f"crf-risk model fc.weight.grad moves by {size:.3e}, err {err:.3e}, tolerance {tol:.3e}")
    assert size > 100 * tol, "the risk term's gradient is too small for this check to see it"
    assert err <= tol
