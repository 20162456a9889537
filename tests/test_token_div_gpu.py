"""The token-level divergence kernels on the MI355X (mtvaf_token_divergence_fwd / _bwd, csrc/consistency.hip) and
engine.TokenDivergenceFunction against the float64 restatement of token_div_cases.py.  Bounds: the small loss kernels' (value and
row values |got - ref| <= 1e-5 |ref| + 1e-6; gradients close(rtol=1e-4) against float64 autograd)."""
import math

import pytest
import torch

import token_div_cases as T
from test_model_gpu import DEV, close

pytestmark = pytest.mark.gpu
OK, ERR_SHAPE, ERR_ARG = 0, -1, -3  # include/mtvaf_hip.h


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def value_close(got, ref, name="loss"):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    err, allowed = (got - ref).abs(), 1e-5 * ref.abs() + 1e-6
    print(f"{name}: max err {float(err.max()):.3e}, smallest margin {float((allowed - err).min()):.3e}")
    assert bool(torch.isfinite(got).all()) and bool((err <= allowed).all()), (name, float(err.max()))


def run_abi(hip, x, y, mask, kind, temperature=1.0, reduction="token_mean", B=1, scale=1.0, upstream=T.UPSTREAM):
    """Both entry points on NaN-prefilled outputs -> (loss [1], row_ws [N], dx, dy)"""
    xg, yg = x.to(DEV).contiguous(), y.to(DEV).contiguous()
    m = None if mask is None else mask.to(DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    loss, rows, dx, dy = nan(1), nan(x.shape[0]), nan(*x.shape), nan(*x.shape)
    how = (hip.TOKEN_DIVERGENCE_KINDS[kind], temperature, hip.TOKEN_DIVERGENCE_REDUCTIONS[reduction], B, scale)
    hip.token_divergence_fwd(xg, yg, m, loss, rows, *how)
    hip.token_divergence_bwd(torch.full((1,), upstream, device=DEV), xg, yg, m, dx, dy, *how)
    return loss, rows, dx, dy


def check_case(hip, shape, mask_name, kind, temperature, reduction):
    x, y, mask, ref, ref_rows, gx, gy = T.reference(shape, mask_name, kind, temperature, reduction)
    loss, rows, dx, dy = run_abi(hip, x, y, mask, kind, temperature, reduction, T.BATCH[shape[0]])
    for t in (loss, rows, dx, dy):  # every element of the NaN-prefilled outputs is written
        assert bool(torch.isfinite(t).all())
    value_close(loss[0], ref)
    value_close(rows, ref_rows, "row_ws")
    close(dx, gx, rtol=1e-4, name="dx")
    close(dy, gy, rtol=1e-4, name="dy")
    if mask is not None:
        dead = (mask == 0).to(DEV)
        assert not bool(rows[dead].any()) and not bool(dx[dead].any()) and not bool(dy[dead].any())  # exact zeros
    return loss, rows, dx, dy


@pytest.mark.parametrize("reduction", T.REDUCTIONS)
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", T.SHAPES, ids=str)
def test_kernels_match_the_float64_restatement(hip, shape, kind, reduction):
    loss, rows, dx, dy = check_case(hip, shape, "none", kind, 1.0, reduction)
    if shape[1] == 1:  # one tag: value 0, gradients exact 0
        assert float(loss) == 0.0 and not bool(dx.any()) and not bool(dy.any())


@pytest.mark.parametrize("temperature", [t for t in T.TEMPERATURES if t != 1.0])
@pytest.mark.parametrize("kind", T.KINDS)
def test_temperature(hip, kind, temperature):
    check_case(hip, (65, 11), "prefix", kind, temperature, "token_mean")


@pytest.mark.parametrize("reduction", T.REDUCTIONS)
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("mask_name", [m for m in T.MASKS if m != "none"])
@pytest.mark.parametrize("shape", [(3, 11), (5, 17), (65, 11), (257, 11)], ids=str)
def test_masks(hip, shape, mask_name, kind, reduction):
    loss, rows, dx, dy = check_case(hip, shape, mask_name, kind, 1.0, reduction)
    if mask_name == "dead":
        assert float(loss) == 0.0 and not bool(dx.any()) and not bool(dy.any())
    # NaN / inf planted in the masked rows: the same bits everywhere
    x, y, mask = T.reference(shape, mask_name, kind, 1.0, reduction)[:3]
    xn, yn = x.clone(), y.clone()
    xn[mask == 0], yn[mask == 0] = float("nan"), float("inf")
    again = run_abi(hip, xn, yn, mask, kind, 1.0, reduction, T.BATCH[shape[0]])
    for a, b in zip((loss, rows, dx, dy), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(5, 16), (5, 17)], ids=str)
def test_unaligned_mask_base(hip, shape):
    """The live-row count reads the mask 16 bytes at a time over its aligned body: a mask that starts at an odd address and is
    longer than one vector counts the same rows."""
    N, C = 67, shape[1]
    x, y = T.make_logits(N, C)
    mask = (torch.arange(N) % 3 != 1).to(torch.uint8)
    ref, ref_rows, gx, gy = T.ref_with_grads(x, y, mask, "sym_kl")
    xg, yg = x.to(DEV), y.to(DEV)
    base = torch.zeros(N + 3, dtype=torch.uint8, device=DEV)
    base[3:] = mask.to(DEV)
    m = base[3:]
    assert m.data_ptr() % 16 == 3 and m.is_contiguous()
    loss, rows, dx, dy = (torch.full(s, float("nan"), device=DEV) for s in ((1,), (N,), (N, C), (N, C)))
    hip.token_divergence_fwd(xg, yg, m, loss, rows, 0, 1.0, 0, 1, 1.0)
    hip.token_divergence_bwd(torch.full((1,), T.UPSTREAM, device=DEV), xg, yg, m, dx, dy, 0, 1.0, 0, 1, 1.0)
    value_close(loss[0], ref)
    close(dx, gx, rtol=1e-4, name="dx")
    close(dy, gy, rtol=1e-4, name="dy")


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_extreme_logits(hip, temperature):
    """Rows +-1e4 * one-hot on different tags: finite everywhere, JS at most log 2, and the values within the bound of the float64
    restatement (sym-KL there is ~1e4 / T: the relative part of the bound carries it)."""
    x, y = T.extreme_logits()
    for kind in T.KINDS:
        ref, ref_rows, gx, gy = T.ref_with_grads(x, y, None, kind, temperature)
        loss, rows, dx, dy = run_abi(hip, x, y, None, kind, temperature)
        for t in (loss, rows, dx, dy):
            assert bool(torch.isfinite(t).all())
        if kind == "js":
            assert float(rows.max()) <= math.log(2.0) * (1 + 1e-6)
        value_close(loss[0], ref, kind)
        value_close(rows, ref_rows, kind + " row_ws")
        close(dx, gx, rtol=1e-4, name="dx")
        close(dy, gy, rtol=1e-4, name="dy")


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", [(65, 11), (7, 63)], ids=str)
def test_the_same_buffer_twice_is_exactly_zero(hip, shape, kind):
    x = T.make_logits(*shape, s=40.0)[0].to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    loss, rows, dx, dy = nan(1), nan(shape[0]), nan(*shape), nan(*shape)
    k = hip.TOKEN_DIVERGENCE_KINDS[kind]
    hip.token_divergence_fwd(x, x, None, loss, rows, k, 1.0, 0, 1, 1.0)
    hip.token_divergence_bwd(torch.ones(1, device=DEV), x, x, None, dx, dy, k, 1.0, 0, 1, 1.0)
    assert float(loss) == 0.0 and not bool(rows.any())
    assert not bool(dx.any()) and not bool(dy.any())  # d = lp - lq and a = lp - lm are 0 in every lane


def test_two_calls_give_the_same_bits(hip):
    x, y = T.make_logits(4096, 11)
    mask = T.make_mask("prefix", 4096)
    for kind in T.KINDS:
        a, b = run_abi(hip, x, y, mask, kind), run_abi(hip, x, y, mask, kind)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_function_argument_forms(hip):
    from mtvaf_amd import engine
    B, S, C = 5, 13, 11
    x, y = T.make_logits(B * S, C)
    mask = T.make_mask("prefix", B * S)
    ref, _, gx, gy = T.ref_with_grads(x, y, mask, "js", 0.5, "batch_mean", B)

    def run(xt, yt, m, *args):
        out = engine.TokenDivergenceFunction.apply(xt, yt, m, *args)
        assert out.dim() == 0 and out.dtype == torch.float32
        (out * T.UPSTREAM).backward()
        return out.detach()

    # [B,S,C] with a [B,S] int64 mask: the batch mean divides by B
    x3, y3 = (t.view(B, S, C).to(DEV).requires_grad_(True) for t in (x, y))
    js = run(x3, y3, mask.view(B, S).long().to(DEV), "js", 0.5, "batch_mean")
    value_close(js, ref)
    close(x3.grad.view(-1, C), gx, rtol=1e-4, name="dx")
    close(y3.grad.view(-1, C), gy, rtol=1e-4, name="dy")
    assert x3.grad.shape == x3.shape
    # a transposed view gives the bits of its contiguous copy
    xt = x.view(B, S, C).to(DEV).transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    yt = y.view(B, S, C).to(DEV).requires_grad_(True)
    assert not xt.is_contiguous()
    jt = run(xt, yt, mask.view(B, S).bool().to(DEV), "js", 0.5, "batch_mean")
    assert torch.equal(jt, js) and torch.equal(xt.grad, x3.grad) and torch.equal(yt.grad, y3.grad)
    # float64 inputs are computed in fp32 and get gradients of their own dtype
    xd = x.double().view(B, S, C).to(DEV).requires_grad_(True)
    jd = run(xd, y.view(B, S, C).to(DEV), mask.view(B, S).to(DEV), "js", 0.5, "batch_mean")
    assert torch.equal(jd, js) and xd.grad.dtype == torch.float64 and torch.equal(xd.grad.float(), x3.grad)
    # scale rides in the kernel
    xq, yq = (t.to(DEV).requires_grad_(True) for t in (x, y))
    jq = run(xq, yq, mask.to(DEV), "js", 0.5, "batch_mean", 0.25)   # [N,C]: B = 1
    value_close(jq, 0.25 * B * ref)
    close(xq.grad, 0.25 * B * gx, rtol=1e-4, name="dx scale 0.25")
    close(yq.grad, 0.25 * B * gy, rtol=1e-4, name="dy scale 0.25")
    # the same tensor twice: exactly 0, two gradients summed by autograd
    xs = x.to(DEV).requires_grad_(True)
    same = engine.TokenDivergenceFunction.apply(xs, xs)
    assert float(same.detach()) == 0.0
    same.backward()
    assert xs.grad is not None and not bool(xs.grad.any())
    with pytest.raises(ValueError):
        engine.TokenDivergenceFunction.apply(xs, xs[:-1])
    with pytest.raises(ValueError):
        engine.TokenDivergenceFunction.apply(xs, xs, None, "kl")
    with pytest.raises(RuntimeError, match="bad shape"):
        z = torch.zeros(4, 65, device=DEV)
        engine.TokenDivergenceFunction.apply(z, z)


def test_error_codes_come_back_before_any_launch(hip):
    lib = hip.lib()
    z = torch.zeros(4, 64, device=DEV)
    out = torch.full((4 * 64 + 5,), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    st = hip._st()

    def fwd(N=4, C=64, kind=0, temp=1.0, red=0, B=1):
        return lib.mtvaf_token_divergence_fwd(p(z), p(z), None, p(out), p(out[1:]), N, C, kind, temp, red, B, 1.0, st)

    def bwd(N=4, C=64, kind=0, temp=1.0, red=0, B=1):
        return lib.mtvaf_token_divergence_bwd(p(out), p(z), p(z), None, p(out[8:]), p(out[8:]), N, C, kind, temp, red, B, 1.0, st)

    for call in (fwd, bwd):
        assert call(C=0) == ERR_SHAPE and call(C=65) == ERR_SHAPE and call(N=0) == ERR_SHAPE
        assert call(temp=0.0) == ERR_ARG and call(temp=-1.0) == ERR_ARG and call(temp=float("nan")) == ERR_ARG
        assert call(temp=float("inf")) == ERR_ARG
        assert call(kind=2) == ERR_ARG and call(kind=-1) == ERR_ARG and call(red=2) == ERR_ARG and call(red=1, B=0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing ran
    assert fwd(C=1, N=4) == OK
