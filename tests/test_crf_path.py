"""CPU-side checks of the path-cost contract: the float64 references of crf_path_cases (expected path cost, entropy, KL) and the
centred restatement with the edge terms against enumeration of all paths, the centred restatement against the reference in
float64 (to 1e-9 of max(1, max|ref|), the rule of test_crf_risk.py), and the host-side argument checks of CRF.expected_path_cost / entropy / kl_divergence."""
import pytest
import torch

import crf_lattice_cases as X
import crf_llh_cases as L
import crf_path_cases as Pc
import crf_wide_cases as W


@pytest.mark.parametrize("case", Pc.BRUTE, ids=str)
def test_references_against_enumeration(case):
    B, S, C, seed, lengths = case
    inp = W.crf_inputs(B, S, C, seed, lengths=list(lengths))
    inp_q = W.crf_inputs(B, S, C, seed + 1, lengths=list(lengths))
    w = L.weights(B)
    shape = (B, S, C, 1)
    for pattern in ("b", "e", "s"):
        cost, ecost = Pc.make_costs(shape, pattern, inp)
        bf = Pc.bruteforce(inp, cost, ecost, w, inp_q)
        for name, got in (("oracle", Pc.oracle(inp, cost, ecost, w)), ("centred", Pc.centred(inp, cost, ecost, w, torch.float64))):
            assert float((got["risk"] - bf["risk"]).abs().max()) <= 1e-12 * max(1.0, float(bf["risk"].abs().max())), name
            for k in ("dem", "dtrans", "decost"):
                assert float((got[k] - bf[k]).abs().max()) <= 1e-12 * max(1.0, float(bf[k].abs().max())), (name, pattern, k)
            assert float((got["decost"] - got["ztrans"]).abs().max()) <= 1e-12
    h = Pc.entropy_oracle(inp, w)
    assert float((h["h"] - bf["entropy"]).abs().max()) <= 1e-12 * max(1.0, float(h["logz"].abs().max()))
    # the entropy's gradient is minus the covariance with the chain's own score (summed in float64: (s) rounds it to float32)
    cost, ecost = Pc.score_cost(tuple(x.double() if x.is_floating_point() else x for x in inp))
    bf = Pc.bruteforce(inp, cost, ecost, w, inp_q)
    for k in ("dem", "dtrans"):
        assert float((h[k] + bf[k]).abs().max()) <= 1e-12 * max(1.0, float(bf[k].abs().max())), k
    c64 = Pc.centred(inp, cost, ecost, w, torch.float64)
    assert float((c64["logz"] - c64["risk"] - bf["entropy"]).abs().max()) <= 1e-12 * max(1.0, float(h["logz"].abs().max()))
    kl = Pc.kl_oracle(inp, inp_q, w)
    assert float((kl["kl"] - bf["kl"]).abs().max()) <= 1e-12 * max(1.0, float(kl["logz"].max()))
    assert float(kl["kl"].min()) >= 0.0


@pytest.mark.parametrize("shape", [s for s in Pc.SHAPES if s[1] <= 65], ids=str)
def test_centred_recursions_are_the_reference_in_float64(shape):
    inp = X.inputs(shape)
    w = L.weights(shape[0])
    for pattern in ("b", "e", "c", "s"):
        cost, ecost = Pc.make_costs(shape, pattern, inp)
        r64, c64 = Pc.oracle(inp, cost, ecost, w), Pc.centred(inp, cost, ecost, w, torch.float64)
        for k in Pc.QUANTITIES:
            # test_crf_risk.py's rule: 1e-9 of max(1, max|ref|), i.e. relative for a quantity above 1 and ABSOLUTE 1e-9 below it.
            # A purely relative 1e-9 is beyond the float64 autograd reference itself where scores reach 1e3 (scale 6): its
            # dend of 2.2e-3 differs from the recursion's by 2.9e-12 = 1.3e-9 of it, every other quantity by less than 5e-10.
            assert float((c64[k] - r64[k]).abs().max()) <= 1e-9 * max(1.0, float(r64[k].abs().max())), (pattern, k)
        if pattern == "s":  # the entropy by autograd through the score's own parameters: minus the covariance gradients
            h = Pc.entropy_oracle(inp, w)
            c64 = Pc.centred(inp, *Pc.score_cost(tuple(x.double() if x.is_floating_point() else x for x in inp)), w, torch.float64)
            assert float((h["h"] - (c64["logz"] - c64["risk"])).abs().max()) <= 1e-9 * max(1.0, float(h["logz"].abs().max()))
            for k in ("dem", "dstart", "dend", "dtrans"):
                assert float((h[k] + c64[k]).abs().max()) <= 1e-9 * max(1.0, float(h[k].abs().max())), k


@pytest.mark.parametrize("shared", [False, True], ids=["other", "shared"])
@pytest.mark.parametrize("shape", [(3, 2, 2, 1), (3, 17, 11, 1)], ids=str)
def test_kl_composition_is_the_reference_in_float64(shape, shared):
    """The engine's composition (cost covariance on p; -(marginals of p) + (marginals of q) on q) against autograd of KL."""
    inp_p, inp_q = Pc.kl_inputs(shape, shared)
    w = L.weights(shape[0])
    r64 = Pc.kl_oracle(inp_p, inp_q, w, shared)
    d = lambda inp: tuple(x.double() if x.is_floating_point() else x for x in inp)
    cp, ecp = Pc.score_cost(d(inp_p))
    cq, ecq = Pc.score_cost(d(inp_q))
    P = Pc.centred(inp_p, cp - cq, ecp - ecq, w, torch.float64)
    Q = Pc.centred(inp_q, None, None, w, torch.float64)
    tol = lambda k: 1e-9 * max(1.0, float(r64[k].abs().max()))
    assert float(((P["risk"] - P["logz"] + Q["logz"]) - r64["kl"]).abs().max()) <= 1e-9 * float(r64["logz"].max())
    assert float((P["dem"] - r64["dem_p"]).abs().max()) <= tol("dem_p")
    assert float((Q["zem"] - P["dcost"] - r64["dem_q"]).abs().max()) <= tol("dem_q")
    both = P["dtrans"] + Q["ztrans"] - P["decost"]
    want = r64["dtrans_p"] if shared else r64["dtrans_p"] + r64["dtrans_q"]
    assert float((both - want).abs().max()) <= tol("dtrans_p")
    assert float(r64["kl"].min()) >= 0.0


@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (3, 65, 11, 6), (3, 2, 64, 1)], ids=str)
def test_centred_float32_meets_the_bounds(shape):
    """The error model passes its own rule (make_reference has asserted that no bound is vacuous)."""
    for pattern in ("b", "s"):
        ref = Pc.reference(shape, pattern)
        for k in Pc.QUANTITIES:
            Pc.check(ref, k, ref.c32[k])
    ref = Pc.entropy_reference(shape)
    for k in ref.c32:
        Pc.check(ref, k, ref.c32[k])
    z = Pc.oracle(X.inputs(shape), *Pc.make_costs(shape, "z", X.inputs(shape)), L.weights(shape[0]))
    assert all(float(z[k].abs().max()) == 0.0 for k in ("risk", "dem", "dstart", "dend", "dtrans"))


def test_path_cost_rejects_bad_arguments():
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(5, batch_first=True)
    em, cost, edge = torch.randn(2, 7, 5), torch.randn(2, 7, 5), torch.randn(5, 5)
    for call in (lambda: crf.expected_path_cost(em, cost, edge, reduction="median"), lambda: crf.entropy(em, reduction="median"),
                 lambda: crf.kl_divergence(em, em, reduction="median")):
        with pytest.raises(ValueError, match="invalid reduction"):
            call()
    with pytest.raises(ValueError, match="does not fit"):
        crf.expected_path_cost(em, cost[:, :6], edge)
    with pytest.raises(ValueError, match="does not fit"):
        crf.expected_path_cost(em, cost, edge[:4])
    with pytest.raises(ValueError, match="floating-point"):
        crf.expected_path_cost(em, cost, torch.ones(5, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="does not fit"):
        crf.kl_divergence(em, em[:, :6])
    with pytest.raises(ValueError, match="tags"):
        crf.kl_divergence(em, em, other=CRF(4, batch_first=True))
    with pytest.raises(ValueError, match="S=513"):
        crf.entropy(torch.randn(1, 513, 5))
    for call in (lambda: crf.expected_path_cost(em, cost, edge), lambda: crf.expected_path_cost(em, None, edge),
                 lambda: crf.entropy(em), lambda: crf.kl_divergence(em, em)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
