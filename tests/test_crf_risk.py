"""CPU-side checks of the expected-cost (risk) contract: the float64 reference of crf_risk_cases against enumeration of all
paths, the centred restatement against the reference (float64: to rounding; float32: inside the bounds, which must not be
vacuous), the two invariants of the contract, and the host-side pieces of CRF.expected_cost / hamming_risk."""
import pytest
import torch

import crf_lattice_cases as X
import crf_llh_cases as L
import crf_risk_cases as R
import crf_wide_cases as W


@pytest.mark.parametrize("case", R.BRUTE, ids=str)
def test_reference_against_enumeration(case):
    B, S, C, seed, lengths = case
    inp = W.crf_inputs(B, S, C, seed, lengths=list(lengths))
    w = L.weights(B)
    for pattern in ("h", "r"):
        cost = R.make_cost((B, S, C, 1), pattern, inp)
        r64 = R.oracle(inp, cost, w)
        risk, dem, dtrans = R.bruteforce(inp, cost, w)
        assert float((r64["risk"] - risk).abs().max()) <= 1e-12 * max(1.0, float(risk.abs().max()))
        assert float((r64["dem"] - dem).abs().max()) <= 1e-12
        assert float((r64["dtrans"] - dtrans).abs().max()) <= 1e-12
        on = R.live(inp[2])
        assert float((r64["dstart"] - (dem[:, 0]).sum(0)).abs().max()) <= 1e-12
        last = dem[torch.arange(B), X.lengths_of(inp[2]) - 1]
        assert float((r64["dend"] - last.sum(0)).abs().max()) <= 1e-12
        assert float((r64["dcost"] - w.double()[:, None, None] * r64["marg"]).abs().max()) <= 1e-12
        assert bool((r64["dem"][~on] == 0).all())


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[1] <= 65], ids=str)
def test_centred_recursions_are_the_reference_in_float64(shape):
    inp = X.inputs(shape)
    w = L.weights(shape[0])
    for pattern in ("h", "r", "k"):
        cost = R.make_cost(shape, pattern, inp)
        r64, c64 = R.oracle(inp, cost, w), R.centred(inp, cost, w, torch.float64)
        for k in R.QUANTITIES:
            assert float((c64[k] - r64[k]).abs().max()) <= 1e-9 * max(1.0, float(r64[k].abs().max())), (pattern, k)


@pytest.mark.parametrize("pattern", ["h", "r"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_centred_float32_meets_the_bounds(shape, pattern):
    """The error model passes its own rule (make_reference has asserted that no bound is vacuous)."""
    ref = R.reference(shape, pattern)
    for k in R.QUANTITIES:
        R.check(ref, k, ref.c32[k])


@pytest.mark.parametrize("shape", [(3, 17, 11, 1), (3, 65, 11, 6), (3, 2, 64, 1)], ids=str)
def test_invariants_of_the_reference(shape):
    """sum_c dR/dem[t,c] = 0 at every column; a per-column constant moves R by its sum over the live columns and no gradient."""
    r = R.reference(shape, "r")
    assert float(r.r64["dem"].sum(-1).abs().max()) <= 1e-9  # (the double backward's own float64 rounding)
    const = R.column_constants(shape).double()  # (added in float64: the float32 sum of pattern (k) is rounded per tag)
    k64 = R.oracle(r.inputs, r.cost.double() + const, r.w)
    shift = (const[..., 0] * R.live(r.inputs[2])).sum(1)
    assert float((k64["risk"] - r.r64["risk"] - shift).abs().max()) <= 1e-9
    for name in ("dem", "dstart", "dend", "dtrans", "dcost"):
        assert float((k64[name] - r.r64[name]).abs().max()) <= 1e-9, name
    z = R.reference(shape, "z")
    assert all(float(z.r64[name].abs().max()) == 0.0 for name in ("risk", "dem", "dstart", "dend", "dtrans"))


def test_hamming_cost_and_reductions():
    from mtvaf_amd.modules.crf import CRF
    tags = torch.tensor([[1, 2, 0, 3], [2, 7, -100, 0]])
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]], dtype=torch.uint8)
    cost, kept = CRF.hamming_cost(tags, 4, mask)
    assert kept.tolist() == [[True] * 4, [True, True, False, False]]
    assert cost.dtype == torch.float32 and cost[0].tolist() == [[1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 0]]
    assert cost[1].tolist() == [[1, 1, 0, 1], [1, 1, 1, 0], [0] * 4, [0] * 4]  # (7 is clamped to the last tag; masked: zeros)
    keep = torch.tensor([[0, 1, 1, 0], [1, 1, 1, 1]], dtype=torch.bool)
    cost, kept = CRF.hamming_cost(tags, 4, mask, keep)
    assert kept.tolist() == [[False, True, True, False], [True, True, False, False]] and int(kept.sum()) == 4
    assert bool((cost[0, 0] == 0).all()) and bool((cost[0, 3] == 0).all()) and cost[0, 1].tolist() == [1, 1, 0, 1]
    with pytest.raises(ValueError):
        CRF.hamming_cost(tags, 4, mask, keep[:, :3])
    # the expected number of wrong tags: sum over kept columns of 1 - m_t(tag), on the reference's marginals
    ref = R.reference((3, 17, 11, 1), "h")
    em, tg, mk = ref.inputs[:3]
    cost, kept = CRF.hamming_cost(tg, 11, mk)
    assert torch.equal(cost, ref.cost)
    want = ((1 - ref.r64["marg"].gather(2, tg[..., None])[..., 0]) * kept).sum(1)
    assert float((want - ref.r64["risk"]).abs().max()) <= 1e-12
    risk = torch.tensor([1.0, 2.0, 4.5])
    assert CRF.reduce_risk(risk, 5.0, "none") is risk
    assert float(CRF.reduce_risk(risk, 5.0, "sum")) == 7.5 and float(CRF.reduce_risk(risk, 5.0, "mean")) == 2.5
    assert float(CRF.reduce_risk(risk, 5.0, "token_mean")) == 1.5
    with pytest.raises(ValueError):
        CRF.reduce_risk(risk, 5.0, "median")


def test_expected_cost_rejects_bad_arguments():
    from mtvaf_amd import hip
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(5, batch_first=True)
    em, cost = torch.randn(2, 7, 5), torch.randn(2, 7, 5)
    with pytest.raises(ValueError, match="invalid reduction"):
        crf.expected_cost(em, cost, reduction="median")
    with pytest.raises(ValueError, match="invalid reduction"):
        crf.hamming_risk(em, torch.zeros(2, 7, dtype=torch.long), reduction="median")
    with pytest.raises(ValueError, match="does not fit"):
        crf.expected_cost(em, cost[:, :6])
    with pytest.raises(ValueError, match="does not fit"):
        crf.expected_cost(em, cost[..., 0])
    with pytest.raises(ValueError, match="floating-point"):
        crf.expected_cost(em, torch.ones(2, 7, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="floating-point"):
        crf.expected_cost(em, cost.tolist())
    with pytest.raises(ValueError):  # C > 64: the module holds at most 64 tags, so such emissions never fit it
        CRF(64, batch_first=True).expected_cost(torch.randn(2, 7, 65), torch.randn(2, 7, 65))
    with pytest.raises(ValueError, match="C=65"):
        hip.crf_risk_check(torch.randn(2, 7, 65), torch.randn(2, 7, 65))
    with pytest.raises(ValueError, match="S=513"):
        crf.expected_cost(torch.randn(1, 513, 5), torch.randn(1, 513, 5))
    with pytest.raises(ValueError, match="S=513"):
        crf.differentiable_marginals(torch.randn(1, 513, 5))
    for call in (lambda: crf.expected_cost(em, cost), lambda: crf.hamming_risk(em, torch.zeros(2, 7, dtype=torch.long)),
                 lambda: crf.differentiable_marginals(em)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
