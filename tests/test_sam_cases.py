"""CPU: the float64 restatement of tests/sam_cases.py is the textbook SAM ascent step, and the case table holds the edges the GPU
tests rely on."""
import math

import torch

import sam_cases as C


def test_reference_is_the_textbook_sam_loop_on_a_two_layer_mlp_in_float64():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).double()
    x, y = torch.randn(11, 7, dtype=torch.float64), torch.randn(11, 3, dtype=torch.float64)
    torch.nn.functional.mse_loss(net(x), y).backward()
    ps = [p.detach().clone() for p in net.parameters()]
    gs = [p.grad.detach().clone() for p in net.parameters()]
    # the loop of the paper: e = rho g / (|g| + 1e-12) with the global norm, p += e
    norm = torch.norm(torch.stack([g.norm(2) for g in gs]), 2)
    rho = float(C.np.float32(C.RHO))  # (the C ABI takes rho as a float)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(p.grad * (rho / (norm + 1e-12)))
    ref = C.reference(ps, gs, rho)
    assert ref["finite"] and abs(ref["norm"] - float(norm)) <= 1e-14 * float(norm)
    for p, p0, want in zip(net.parameters(), ps, ref["p_new"]):
        assert torch.allclose(want.reshape(p.shape), p.detach(), rtol=0, atol=1e-14) and not torch.equal(p.detach(), p0)


def test_case_table_holds_the_edges():
    assert {1, 3, 4, 5, 65532, 65536, 65540} <= set(C.SIZES) and C.CHUNK == 65536
    ns = [c["n"] for c in C.CASES]
    assert set(C.SIZES) <= set(ns)
    kinds = {c["kind"] for c in C.CASES}
    assert {"scaled-down", "scaled-up", "zero", "overflow32", "inf", "nan"} <= kinds
    assert any(off for _, off in C.MULTI) and any(not off for _, off in C.MULTI) and set(C.SIZES) <= {n for n, _ in C.MULTI}
    for c in C.CASES:
        p, g = C.make_inputs(c["n"], c["kind"])
        norm = C.ordered_norm64(C.host_partials([g]))
        if c["kind"] in ("randn", "scaled-down", "scaled-up"):
            assert math.isfinite(norm) and norm > 0 and C.fits32(norm), c["id"]
        elif c["kind"] == "zero":
            assert norm == 0.0 and float(C.scale32(C.RHO, norm)) * 0.0 == 0.0
        elif c["kind"] == "overflow32":
            assert math.isfinite(norm) and not C.fits32(norm), c["id"]  # finite in double, not in fp32
        else:
            assert not math.isfinite(norm)


def test_half_ulp_measure():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -23, 3.0], dtype=torch.float32)
    exact = x.double() + torch.tensor([2.0 ** -25, -2.0 ** -25, 2.0 ** -23], dtype=torch.float64)
    assert abs(C.half_ulp_excess(x, exact) - 1.0) < 1e-12  # 2^-23 off at 3.0 (ulp 2^-22) is exactly half an ulp
    assert C.half_ulp_excess(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64)) == float("inf")
