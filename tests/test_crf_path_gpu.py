"""The path-cost entry points (mtvaf_crf_path_{fwd,bwd}) and the layers above them -- engine.CRFPathFunction / CRFEntropyFunction /
CRFKLFunction, CRF.expected_path_cost / entropy / kl_divergence, TVNetSAModel2's args.crf_entropy_weight -- on the MI355X, against
the float64 references under the acceptance rule of crf_path_cases.

Largest err / bound per quantity over this file, one run on one MI355X.  C ABI: risk 0.039, logz 0.004,
dem 0.029, dstart 0.248, dend 0.248, dtrans 0.201, dcost 0.003, decost 0.007 (dtrans: 2.8e-5 on a bound of 1.4e-4 at (3,512,64,1)
with the chain's own score as cost; dstart / dend: 3.2e-7 on a bound of 1.3e-6); gz gradients 0.007 at most; entropy 0.005, its gradients 0.029 / 0.305 /
0.305 / 0.201 (dem / dstart / dend / dtrans); KL over the same shapes, other and shared parameters: value 0.007, p side 0.005 / 0.330 /
0.330 / 0.092, q side 0.005 / 0.010 / 0.010 / 0.010."""
import math

import pytest
import torch

import crf_lattice_cases as X
import crf_path_cases as Pc
import crf_risk_cases as R
import params as P
from test_crf_lattice_gpu import tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _run(hip, inp, cost, ecost, w, gz=None, accumulate=False, fill=(0.0, 0.0, 0.0, 0.0), want_dcost=True, want_decost=True,
         want_logz=True):
    em, _, mask, start, end, trans = _dev(*inp)
    cost, ecost, w, gz = _dev(cost, ecost, w, gz)
    B, S, C = em.shape
    ws, wsb = hip.crf_path_workspace(B, S, C, DEV)
    full = lambda shape, v=7.0: torch.full(shape, v, device=DEV)
    risk, logz = full((B,)), full((B,)) if want_logz else None
    hip.crf_path_fwd(em, cost, ecost, mask, start, end, trans, risk, logz, ws, wsb)
    dem = full((B, S, C))
    dcost = full((B, S, C)) if want_dcost else None
    decost = full((C, C), fill[3]) if want_decost else None
    ds, de, dt = full((C,), fill[0]), full((C,), fill[1]), full((C, C), fill[2])
    hip.crf_path_bwd(w, gz, em, cost, ecost, mask, start, end, trans, dem, dcost, decost, ds, de, dt, accumulate, ws, wsb)
    return dict(risk=risk, logz=logz, dem=dem, dcost=dcost, decost=decost, dstart=ds, dend=de, dtrans=dt)


def _crf(C, start, end, trans, batch_first=True):
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(C, batch_first=batch_first).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start), crf.end_transitions.copy_(end), crf.transitions.copy_(trans)
    return crf


def _pos_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["b", "e", "c", "s"])
@pytest.mark.parametrize("shape", Pc.SHAPES, ids=str)
def test_fwd_bwd_abi(hip, shape, pattern):
    ref = Pc.reference(shape, pattern)
    B = shape[0]
    got = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w)
    for name in ("risk", "logz") + Pc.GRADS:
        Pc.check(ref, name, got[name])
    on = Pc.live(ref.inputs[2])
    dem, dcost = got["dem"].cpu(), got["dcost"].cpu()
    assert _pos_zero(dem[~on]) and _pos_zero(dcost[~on])
    if B >= 2:
        assert float(ref.w[1]) == 0.0 and _pos_zero(dem[1]) and _pos_zero(dcost[1])
    colsum = float(dem.double().sum(-1)[on].abs().max())
    print(f"crf-path column sum of dem {colsum:.3e} (bound {ref.bound['dem']:.3e})")
    assert colsum <= ref.bound["dem"]
    again = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    if pattern == "c":  # ecost == NULL: inside crf_risk_cases' bounds for the same node cost
        rref = R.reference(shape, "r")
        assert torch.equal(rref.cost, ref.cost)
        for name in ("risk", "logz", "dem", "dstart", "dend", "dtrans", "dcost"):
            R.check(rref, name, got[name])


@pytest.mark.parametrize("shape", Pc.SHAPES, ids=str)
def test_zero_cost_masked_nan_and_logz_gradient(hip, shape):
    ref = Pc.reference(shape, "b")
    got = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w)
    # (z) nothing is paid and nothing moves, exactly: explicit zeros, and both costs NULL
    zc, ze = Pc.make_costs(shape, "z", ref.inputs)
    for cost, ecost in ((zc, ze), (None, None), (zc, None), (None, ze)):
        zero = _run(hip, ref.inputs, cost, ecost, ref.w)
        for name in ("risk", "dem", "dstart", "dend", "dtrans"):  # (+0.0, also under the negative and the zero weights)
            assert _pos_zero(zero[name]), name
    # (n) NaN at the masked columns of the node cost is never read
    nc, ne = Pc.make_costs(shape, "n", ref.inputs)
    nan = _run(hip, ref.inputs, nc, ne, ref.w)
    for name in got:
        assert bool(torch.isfinite(nan[name]).all()) and torch.equal(nan[name], got[name]), name
    # NaN at the masked columns of the emissions is never read either
    em_nan = torch.where(Pc.live(ref.inputs[2])[..., None], ref.inputs[0], torch.full_like(ref.inputs[0], float("nan")))
    nan = _run(hip, (em_nan,) + tuple(ref.inputs[1:]), nc, ne, ref.w)
    for name in got:
        assert bool(torch.isfinite(nan[name]).all()) and torch.equal(nan[name], got[name]), name
    # both costs NULL with gz = w: w times the gradient of logZ; a sentence with grad == gz == 0 gets zeros
    z = _run(hip, ref.inputs, None, None, torch.zeros_like(ref.w), gz=ref.w, want_dcost=False, want_decost=False)
    for name, zname in (("dem", "zem"), ("dstart", "zstart"), ("dend", "zend"), ("dtrans", "ztrans")):
        Pc.check(ref, zname, z[name])
    if shape[0] >= 2:
        assert _pos_zero(z["dem"][1])
    assert _pos_zero(z["dem"].cpu()[~Pc.live(ref.inputs[2])])
    # grad and gz together: the sum of the two gradients
    both = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w, gz=ref.w)
    for name, zname in (("dem", "zem"), ("dstart", "zstart"), ("dend", "zend"), ("dtrans", "ztrans")):
        err = float((both[name].double().cpu() - ref.r64[name] - ref.r64[zname]).abs().max())
        assert err <= ref.bound[name] + ref.bound[zname], name
    assert torch.equal(both["decost"], got["decost"]) and torch.equal(both["dcost"], got["dcost"])


def test_accumulate_and_optional_outputs(hip):
    ref = Pc.reference((3, 17, 11, 1), "b")
    got = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w, accumulate=True, fill=(0.5, -2.0, 3.0, -1.5))
    Pc.check(ref, "dstart", got["dstart"], add=0.5)
    Pc.check(ref, "dend", got["dend"], add=-2.0)
    Pc.check(ref, "dtrans", got["dtrans"], add=3.0)
    Pc.check(ref, "decost", got["decost"], add=-1.5)
    plain = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w)
    bare = _run(hip, ref.inputs, ref.cost, ref.ecost, ref.w, want_dcost=False, want_decost=False, want_logz=False)
    for name in ("risk", "dem", "dstart", "dend", "dtrans"):  # logz, dcost and decost are optional
        assert torch.equal(bare[name], plain[name]), name


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
    assert lib.mtvaf_crf_path_workspace_bytes(B, S, C) == 0
    assert lib.mtvaf_crf_path_fwd(p(em), p(em), p(trans), p(mask), p(start), p(end), p(trans), p(out), None, B, S, C, p(ws),
                                  ws.numel(), st) == -1
    assert lib.mtvaf_crf_path_bwd(p(out), None, p(em), p(em), p(trans), p(mask), p(start), p(end), p(trans), p(dem), None, None,
                                  p(start), p(end), p(trans), 0, B, S, C, p(ws), ws.numel(), st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((dem == 7).all()) and int(ws.sum()) == 0


def test_small_workspace_is_refused(hip):
    ref = Pc.reference((3, 17, 11, 1), "b")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    cost, ecost, w = _dev(ref.cost, ref.ecost, ref.w)
    ws, wsb = hip.crf_path_workspace(3, 17, 11, DEV)
    risk, dem = torch.full((3,), 7.0, device=DEV), torch.full((3, 17, 11), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="mtvaf_crf_path_fwd failed: workspace too small"):
        hip.crf_path_fwd(em, cost, ecost, mask, start, end, trans, risk, None, ws, wsb - 4)
    with pytest.raises(RuntimeError, match="mtvaf_crf_path_bwd failed: workspace too small"):
        hip.crf_path_bwd(w, None, em, cost, ecost, mask, start, end, trans, dem, None, None, start.clone(), end.clone(),
                         trans.clone(), False, ws, wsb - 4)
    torch.cuda.synchronize()
    assert bool((risk == 7).all()) and bool((dem == 7).all())


# ---- 2. autograd and the module ----------------------------------------------------------------------------------------------
def test_expected_path_cost_autograd():
    shape = (3, 17, 11, 1)
    ref = Pc.reference(shape, "b")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    cost, ecost, w = _dev(ref.cost, ref.ecost, ref.w)
    n = float(mask.sum())
    for batch_first in (True, False):
        crf = _crf(11, start, end, trans, batch_first)
        lay = (lambda x: x) if batch_first else (lambda x: x.transpose(0, 1))
        e, c, ec = lay(em).clone().requires_grad_(True), lay(cost).clone().requires_grad_(True), ecost.clone().requires_grad_(True)
        risk = crf.expected_path_cost(e, c, ec, lay(mask))
        Pc.check(ref, "risk", risk)
        (risk * w).sum().backward()
        Pc.check(ref, "dem", lay(e.grad))
        Pc.check(ref, "dcost", lay(c.grad))
        Pc.check(ref, "decost", ec.grad)
        Pc.check(ref, "dstart", crf.start_transitions.grad)
        Pc.check(ref, "dend", crf.end_transitions.grad)
        Pc.check(ref, "dtrans", crf.transitions.grad)
        r64 = ref.r64["risk"]
        for red, want, scale in (("sum", r64.sum(), 3.0), ("mean", r64.mean(), 1.0), ("token_mean", r64.sum() / n, 1.0)):
            got = float(crf.expected_path_cost(lay(em), lay(cost), ecost, lay(mask), reduction=red).detach())
            assert abs(got - float(want)) <= ref.bound["risk"] * scale, red
    eref = Pc.reference(shape, "e")  # either cost may be None; a cost that asks for no gradient gets none
    e = em.clone().requires_grad_(True)
    Pc.check(eref, "risk", crf.expected_path_cost(lay(e), None, ecost, lay(mask)))
    crf.expected_path_cost(lay(e), lay(cost), ecost, lay(mask), reduction="sum").backward()
    assert e.grad is not None and cost.grad is None and ecost.grad is None


@pytest.mark.parametrize("shape", Pc.SHAPES, ids=str)
def test_entropy(shape):
    ref = Pc.entropy_reference(shape)
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    B, S, C, _ = shape
    crf = _crf(C, start, end, trans)
    e = em.clone().requires_grad_(True)
    h = crf.entropy(e, mask)
    Pc.check(ref, "h", h, tag="entropy")
    (h * ref.w.to(DEV)).sum().backward()
    Pc.check(ref, "dem", e.grad, tag="entropy dem")
    Pc.check(ref, "dstart", crf.start_transitions.grad, tag="entropy dstart")
    Pc.check(ref, "dend", crf.end_transitions.grad, tag="entropy dend")
    Pc.check(ref, "dtrans", crf.transitions.grad, tag="entropy dtrans")
    lens = X.lengths_of(ref.inputs[2]).double()
    hd, bnd = h.detach().double().cpu(), ref.bound["h"]
    assert bool((hd >= -bnd).all()) and bool((hd <= lens * math.log(C) + bnd).all())
    if C == 1:
        assert float(hd.abs().max()) <= bnd
    n = float(mask.sum())
    for red, want, scale in (("sum", ref.r64["h"].sum(), B), ("mean", ref.r64["h"].mean(), 1.0),
                             ("token_mean", ref.r64["h"].sum() / n, B / n)):
        assert abs(float(crf.entropy(em, mask, reduction=red).detach()) - float(want)) <= bnd * scale, red
    # emissions at masked columns are never read, although the cost is cloned from them: NaN there changes no bit
    on = Pc.live(ref.inputs[2])[..., None].to(DEV)
    e2 = torch.where(on, em, torch.full_like(em, float("nan"))).requires_grad_(True)
    h2 = crf.entropy(e2, mask)
    assert torch.equal(h2.detach(), h.detach())
    (h2 * ref.w.to(DEV)).sum().backward()
    assert torch.equal(e2.grad, e.grad)
    # all parameters and emissions zero: the uniform distribution over C^len paths
    flat = _crf(C, torch.zeros(C), torch.zeros(C), torch.zeros(C, C))
    hu = flat.entropy(torch.zeros_like(em), mask).detach().double().cpu()
    ubnd = 2e-5 * max(float((lens * math.log(C)).max()), 1e-30) if C > 1 else 0.0  # (T_proj at max|logZ| = max len log C)
    assert float((hu - lens * math.log(C)).abs().max()) <= ubnd
    if shape == (3, 17, 11, 1):  # time-major layout
        tm = _crf(C, start, end, trans, batch_first=False)
        assert torch.equal(tm.entropy(em.transpose(0, 1), mask.transpose(0, 1)), h.detach())


@pytest.mark.parametrize("shared", [False, True], ids=["other", "shared"])
@pytest.mark.parametrize("shape", Pc.SHAPES, ids=str)
def test_kl_divergence(shape, shared):
    ref = Pc.kl_reference(shape, shared)
    C = shape[2]
    ep, _, mask, sp, endp, tp = _dev(*ref.p)
    eq, _, _, sq, endq, tq = _dev(*ref.q)
    p = _crf(C, sp, endp, tp)
    q = None if shared else _crf(C, sq, endq, tq)
    a, b = ep.clone().requires_grad_(True), eq.clone().requires_grad_(True)
    kl = p.kl_divergence(a, b, mask, other=q)
    Pc.check(ref, "kl", kl)
    assert float(kl.detach().min()) >= -ref.bound["kl"]
    (kl * ref.w.to(DEV)).sum().backward()
    Pc.check(ref, "dem_p", a.grad, tag="kl dem_p")
    Pc.check(ref, "dem_q", b.grad, tag="kl dem_q")
    for name, par in (("dstart", "start_transitions"), ("dend", "end_transitions"), ("dtrans", "transitions")):
        Pc.check(ref, name + "_p", getattr(p, par).grad, tag="kl " + name + "_p")
        if not shared:
            Pc.check(ref, name + "_q", getattr(q, par).grad, tag="kl " + name + "_q")
    # NaN in the masked columns of either side's emissions changes no bit of the value or of the emissions' gradients
    on = Pc.live(ref.p[2])[..., None].to(DEV)
    nan = torch.full_like(ep, float("nan"))
    a3, b3 = torch.where(on, ep, nan).requires_grad_(True), torch.where(on, eq, nan).requires_grad_(True)
    kl3 = p.kl_divergence(a3, b3, mask, other=q)
    assert torch.equal(kl3.detach(), kl.detach())
    (kl3 * ref.w.to(DEV)).sum().backward()
    assert torch.equal(a3.grad, a.grad) and torch.equal(b3.grad, b.grad)
    # a detached q receives no gradient (and costs no backward call of its own)
    for par in (p if shared else q).parameters():
        par.grad = None
    a2 = ep.clone().requires_grad_(True)
    if shared:
        frozen = _crf(C, sp, endp, tp).requires_grad_(False)
        p.kl_divergence(a2, eq, mask, other=frozen, reduction="sum").backward()
        assert all(par.grad is None for par in frozen.parameters())
    else:
        q.requires_grad_(False)
        p.kl_divergence(a2, eq, mask, other=q, reduction="sum").backward()
        assert all(par.grad is None for par in q.parameters())
    assert a2.grad is not None and eq.grad is None


@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (1, 65, 64, 1)], ids=str)
def test_kl_of_a_chain_with_itself_is_zero(shape):
    ref = Pc.kl_reference(shape, True)
    C = shape[2]
    ep, _, mask, sp, endp, tp = _dev(*ref.p)
    p = _crf(C, sp, endp, tp)
    a, b = ep.clone().requires_grad_(True), ep.clone().requires_grad_(True)
    kl = p.kl_divergence(a, b, mask)
    assert bool((kl == 0).all())
    (kl * ref.w.to(DEV)).sum().backward()
    # the exact gradient is zero on both sides; the p side is an exact +0.0 (zero cost), the q side a difference of two
    # separately rounded marginals, held to the marginals' bound
    assert bool((a.grad == 0).all())
    zb = Pc.reference(shape, "s").bound
    assert float(b.grad.abs().max()) <= 2 * zb["zem"]
    assert float(p.transitions.grad.abs().max()) <= 2 * zb["ztrans"]
    assert float(p.start_transitions.grad.abs().max()) <= 2 * zb["zstart"]
    assert float(p.end_transitions.grad.abs().max()) <= 2 * zb["zend"]


# ---- 3. the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unpad", [False, True], ids=["padded", "padding-free"])
@pytest.mark.parametrize("reduction", ["mean", "token_mean"])
def test_model_crf_entropy_weight(unpad, reduction):
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
        m.args.crf_entropy_weight = weight
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
        assert not hasattr(m.args, "crf_entropy_weight")
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        out = m.train()(**kw)
        out.loss.backward()
        loss_p, g_p = out.loss.detach().clone(), m.fc.weight.grad.detach().clone()  # the parent's path: no such argument
        assert m.last_crf_entropy is None
        loss_0, g_0 = step(0.0)
        assert torch.equal(loss_0, loss_p) and torch.equal(g_0, g_p) and m.last_crf_entropy is None
        loss_h, g_h = step(0.5)
    finally:
        del engine.LinearFunction.apply  # (back to the inherited classmethod)
        engine.UNPAD = was
    # float64 reference of the token-mean entropy on the model's own emissions
    em, h = seen["em"].float().cpu(), seen["h"].double().cpu()
    crf = m.crf
    inp = (em, labels.cpu(), mask.cpu().to(torch.uint8), crf.start_transitions.detach().cpu(), crf.end_transitions.detach().cpu(),
           crf.transitions.detach().cpu())
    n = float(mask.sum())
    w = torch.full((B,), 1.0 / n)
    r64 = Pc.entropy_oracle(inp, w)
    c32 = Pc.centred(inp, *Pc.score_cost(inp), w)
    hbnd = Pc.bound("h", r64["h"], c32["logz"] - c32["risk"], float(r64["logz"].abs().max()))
    rate = float(r64["h"].sum()) / n
    assert m.last_crf_entropy is not None and m.last_crf_entropy.is_cuda and not m.last_crf_entropy.requires_grad
    bnd = hbnd * B / n
    print(f"crf-path model entropy {float(m.last_crf_entropy):.6f} vs {rate:.6f}; loss {float(loss_h):.6f} = {float(loss_0):.6f} + half of it")
    assert abs(float(m.last_crf_entropy) - rate) <= bnd
    # loss_0 and loss_h share the seed and the likelihood term bit for bit; loss_h is ONE float32 of their sum, so beside the
    # entropy bound there is only that number's own rounding, one ulp = 2^-23 |loss_h|
    ulp = 2.0 ** -23
    assert abs(float(loss_h) - (float(loss_0) + 0.5 * rate)) <= bnd + ulp * abs(float(loss_h))
    # the gradient moves by the chain rule's amount: 3e-3 max-norm relative to THAT amount (not to the whole gradient, which
    # the likelihood dominates), plus one ulp of each of the two float32 gradients whose difference is taken
    delta = 0.5 * torch.einsum("bsc,bsh->ch", r64["dem"], h)
    moved = (g_h - g_0).double().cpu()
    err, size = float((moved - delta).abs().max()), float(delta.abs().max())
    tol = 3e-3 * size + 2 * ulp * float(g_h.abs().max())
    print(f"crf-path model fc.weight.grad moves by {size:.3e}, err {err:.3e}, tolerance {tol:.3e}")
    assert size > 100 * tol, "the entropy term's gradient is too small for this check to see it"
    assert err <= tol
