"""The token cross-entropy kernels on the MI355X (mtvaf_token_ce_fwd / _bwd / mtvaf_token_argmax, csrc/token_ce.hip),
engine.TokenCEFunction and modules.token_head.TokenCrossEntropy against the float64 restatement of token_ce_cases.py.  Bounds: the
small loss kernels' (value and row values |got - ref| <= 1e-5 |ref| + 1e-6; gradients close(rtol=1e-4) against float64 autograd)."""
import pytest
import torch

import token_ce_cases as T
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


def run_abi(hip, z, labels, mask=None, weight=None, smoothing=0.0, gamma=0.0, reduction="mean", B=1, scale=1.0,
            upstream=T.UPSTREAM, grad_rows=None):
    """Both entry points on NaN-prefilled outputs -> (loss [1], row_ws [N], stats [2], dlogits)"""
    zg, lg = z.to(DEV).contiguous(), labels.to(DEV)
    m = None if mask is None else mask.to(DEV)
    w = None if weight is None else weight.to(DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    loss, rows, dz = nan(1), nan(z.shape[0]), nan(*z.shape)
    stats = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    how = (T.IGNORE, smoothing, gamma, hip.TOKEN_CE_REDUCTIONS[reduction], B, scale)
    hip.token_ce_fwd(zg, lg, m, w, loss, rows, stats, *how)
    if grad_rows is None:
        hip.token_ce_bwd(torch.full((1,), upstream, device=DEV), None, zg, lg, m, w, dz, *how)
    else:
        hip.token_ce_bwd(None, grad_rows.to(DEV), zg, lg, m, w, dz, *how)
    return loss, rows, stats, dz


def check_case(hip, shape, mask_name, weighted, smoothing, gamma, reduction):
    z, labels, mask, weight, ref, ref_rows, gz = T.reference(shape, mask_name, weighted, smoothing, gamma, reduction)
    loss, rows, stats, dz = run_abi(hip, z, labels, mask, weight, smoothing, gamma, reduction, T.BATCH[shape[0]])
    for t in (loss, rows, dz):  # every element of the NaN-prefilled outputs is written
        assert bool(torch.isfinite(t).all())
    value_close(loss[0], ref)
    value_close(rows, ref_rows, "row_ws")
    close(dz, gz, rtol=1e-4, name="dlogits")
    live = T.live_rows(labels, mask, shape[1])
    dead = (~live).to(DEV)
    assert not bool(rows[dead].any()) and not bool(dz[dead].any())  # exact zeros
    assert stats.tolist() == [int(live.sum()), 0]
    return loss, rows, stats, dz


@pytest.mark.parametrize("gamma", T.GAMMAS)
@pytest.mark.parametrize("smoothing", T.SMOOTHINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", T.SHAPES, ids=str)
def test_kernels_match_the_float64_restatement(hip, shape, weighted, smoothing, gamma):
    loss, rows, stats, dz = check_case(hip, shape, "none", weighted, smoothing, gamma, "mean")
    if shape[1] == 1:  # one tag: value 0, gradients exact 0
        assert float(loss) == 0.0 and not bool(dz.any())


@pytest.mark.parametrize("reduction", T.REDUCTIONS)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("mask_name", [m for m in T.MASKS if m != "none"])
@pytest.mark.parametrize("shape", [(3, 11), (5, 17), (65, 11), (1025, 11)], ids=str)
def test_masks_and_reductions(hip, shape, mask_name, gamma, reduction):
    loss, rows, stats, dz = check_case(hip, shape, mask_name, True, 0.1, gamma, reduction)
    z, labels, mask, weight = T.reference(shape, mask_name, True, 0.1, gamma, reduction)[:4]
    live = T.live_rows(labels, mask, shape[1])
    if not bool(live.any()):
        assert float(loss) == 0.0 and not bool(dz.any()) and stats.tolist() == [0, 0]
    # NaN / inf planted in the dead rows: the same bits everywhere
    zn = z.clone()
    zn[~live] = float("nan")
    zn[~live, 0] = float("inf")
    again = run_abi(hip, zn, labels, mask, weight, 0.1, gamma, reduction, T.BATCH[shape[0]])
    for a, b in zip((loss, rows, stats, dz), again):
        assert torch.equal(a, b)


def test_all_live_weights_zero_give_zero(hip):
    """'mean' with D = 0 although rows are live (every class weight 0): loss 0, all-zero rows and gradients, the rows counted."""
    z, labels = T.make_logits(65, 11), T.make_labels(65, 11)
    loss, rows, stats, dz = run_abi(hip, z, labels, None, torch.zeros(11), 0.0, 0.0, "mean")
    assert float(loss) == 0.0 and not bool(dz.any()) and not bool(rows.any()) and stats.tolist()[0] == 52


def test_out_of_range_labels_are_dead_and_counted(hip):
    N, C = 65, 11
    z, labels, mask, weight = T.make_logits(N, C), T.make_labels(N, C), T.make_mask("prefix", N), T.make_weights(C)
    labels = labels.clone()
    planted = [i for i in range(N) if mask[i] and labels[i] != T.IGNORE][:2]
    labels[planted[0]], labels[planted[1]] = C, -1
    hidden = next(i for i in range(N) if not mask[i])
    labels[hidden] = 10 ** 12   # behind the mask: not looked at
    ref, ref_rows, gz = T.ref_with_grads(z, labels, mask, weight, 0.1, 2.0)
    loss, rows, stats, dz = run_abi(hip, z, labels, mask, weight, 0.1, 2.0)
    live = T.live_rows(labels, mask, C)
    assert stats.tolist() == [int(live.sum()), 2]
    value_close(loss[0], ref)
    value_close(rows, ref_rows, "row_ws")
    close(dz, gz, rtol=1e-4, name="dlogits")
    assert not bool(dz[planted].any()) and not bool(rows[planted].any())


@pytest.mark.parametrize("gamma", [0.0, 3.5])
@pytest.mark.parametrize("shape", [(65, 11), (7, 63)], ids=str)
def test_grad_rows_is_the_none_form(hip, shape, gamma):
    N, C = shape
    z, labels, mask, weight = T.make_logits(N, C), T.make_labels(N, C), T.make_mask("prefix", N), T.make_weights(C)
    g = torch.Generator().manual_seed(5)
    up = torch.randn(N, generator=g)
    live = T.live_rows(labels, mask, C)
    zd = z.double().requires_grad_(True)
    rows64 = T.row_values(zd, labels, live, weight, 0.1, gamma)
    (gz,) = torch.autograd.grad((rows64 * up.double()).sum(), (zd,))
    upn = up.clone()
    upn[~live] = float("nan")  # not read on dead rows
    _, rows, _, dz = run_abi(hip, z, labels, mask, weight, 0.1, gamma, "sum", grad_rows=upn)
    value_close(rows, rows64.detach(), "row_ws")
    assert bool(torch.isfinite(dz).all()) and not bool(dz[(~live).to(DEV)].any())
    close(dz, gz, rtol=1e-4, name="dlogits (grad_rows)")


@pytest.mark.parametrize("smoothing", T.SMOOTHINGS)
@pytest.mark.parametrize("gamma", T.GAMMAS)
def test_extreme_logits(hip, gamma, smoothing):
    """Rows +-1e4 * one-hot with the label on and off the marked tag: finite everywhere and within the bounds of the float64
    restatement (ce is ~1e4 off the peak: the relative part of the bound carries it).  With the label on the peak every other
    tag underflows: om = 0 exactly, so the focal value and gradient of that row are exact zeros."""
    z, labels = T.extreme_logits()
    ref, ref_rows, gz = T.ref_with_grads(z, labels, None, None, smoothing, gamma, "sum")
    loss, rows, stats, dz = run_abi(hip, z, labels, None, None, smoothing, gamma, "sum")
    for t in (loss, rows, dz):
        assert bool(torch.isfinite(t).all())
    value_close(loss[0], ref)
    value_close(rows, ref_rows, "row_ws")
    close(dz, gz, rtol=1e-4, name="dlogits")
    if gamma > 0:
        assert float(rows[0]) == 0.0 and not bool(dz[0].any())


def test_two_calls_give_the_same_bits(hip):
    z, labels, mask, weight = T.make_logits(4096, 11), T.make_labels(4096, 11), T.make_mask("prefix", 4096), T.make_weights(11)
    for gamma in (0.0, 2.0):
        a, b = (run_abi(hip, z, labels, mask, weight, 0.1, gamma) for _ in range(2))
        for u, v in zip(a, b):
            assert torch.equal(u, v)


@pytest.mark.parametrize("shape", [(3, 11), (5, 16), (5, 17), (7, 63), (2, 64), (257, 11), (65, 1)], ids=str)
def test_argmax(hip, shape):
    N, C = shape
    z, mask = T.tied_logits(N, C), T.make_mask("prefix", N)
    zg = z.to(DEV)
    lp64 = torch.log_softmax(z.double(), -1)
    first = torch.stack([(row == row.max()).nonzero()[0, 0] for row in z])   # first index among exact ties
    assert torch.equal(first, torch.argmax(z, -1))   # (the host's argmax takes the first of equal maxima)

    def run(m, allowed):
        tags = torch.full((N,), -9, dtype=torch.int64, device=DEV)
        logp = torch.full((N,), float("nan"), device=DEV)
        hip.token_argmax(zg, None if m is None else m.to(DEV), None if allowed is None else allowed.to(DEV), tags, logp)
        return tags.cpu(), logp.cpu()

    tags, logp = run(None, None)
    assert torch.equal(tags, first)
    value_close(logp, lp64[torch.arange(N), first], "logp")
    # masked rows: tag 0, logp 0, never read
    zn = zg.clone()
    zn[(mask == 0).to(DEV)] = float("nan")
    tags_m = torch.full((N,), -9, dtype=torch.int64, device=DEV)
    logp_m = torch.full((N,), float("nan"), device=DEV)
    hip.token_argmax(zn, mask.to(DEV), None, tags_m, logp_m)
    live = mask != 0
    assert torch.equal(tags_m.cpu(), torch.where(live, first, torch.zeros_like(first)))
    assert torch.equal(logp_m.cpu(), torch.where(live, logp, torch.zeros_like(logp)))
    # allowed sets: the maximum over the permitted tags, the unconstrained log-probability; 0 and bits past C = no constraint
    from mtvaf_amd.constraints import tag_word
    g = torch.Generator().manual_seed(N + C)
    member = torch.rand(N, C, generator=g) < 0.4
    member[1 % N] = False                              # the empty set: unconstrained
    words = torch.tensor([tag_word([j for j in range(C) if member[r, j]]) for r in range(N)], dtype=torch.int64)
    if C < 64:
        words[0] |= tag_word([C])                      # a bit past the tags is ignored
    tags_a, logp_a = run(None, words)
    open_rows = ~member.any(-1)
    zc = torch.where(member | open_rows[:, None], z, torch.full_like(z, float("-inf")))
    want = torch.stack([(row == row.max()).nonzero()[0, 0] for row in zc])
    assert torch.equal(tags_a, want)
    assert bool((member[torch.arange(N), tags_a] | open_rows).all())
    value_close(logp_a, lp64[torch.arange(N), want], "logp (allowed)")


def test_function_and_module_forms(hip):
    from mtvaf_amd import engine
    from mtvaf_amd.modules.token_head import TokenCrossEntropy
    B, S, C = 5, 13, 11
    z, labels, mask, weight = T.make_logits(B * S, C), T.make_labels(B * S, C), T.make_mask("prefix", B * S), T.make_weights(C)
    ref, ref_rows, gz = T.ref_with_grads(z, labels, mask, weight, 0.1, 2.0, "batch_mean", B)
    head = TokenCrossEntropy(C, class_weight=weight.tolist(), smoothing=0.1, focal_gamma=2.0).to(DEV)
    z3 = z.view(B, S, C).to(DEV).requires_grad_(True)
    out = head(z3, labels.view(B, S).to(DEV), mask.view(B, S).long().to(DEV), "batch_mean")
    assert out.dim() == 0 and out.dtype == torch.float32
    (out * T.UPSTREAM).backward()
    value_close(out, ref)
    close(z3.grad.view(-1, C), gz, rtol=1e-4, name="dlogits")
    live = T.live_rows(labels, mask, C)
    assert head.last_stats.dtype == torch.int32 and head.last_stats.tolist() == [int(live.sum()), 0]
    # float64 logits are computed in fp32 and get gradients of their own dtype; a u8 mask gives the same bits
    zd = z.double().view(B, S, C).to(DEV).requires_grad_(True)
    od = head(zd, labels.view(B, S).to(DEV), mask.view(B, S).to(DEV), "batch_mean")
    (od * T.UPSTREAM).backward()
    assert torch.equal(od, out.detach()) and zd.grad.dtype == torch.float64 and torch.equal(zd.grad.float(), z3.grad)
    # "none": rows in the shape of the labels, differentiable per row
    g = torch.Generator().manual_seed(9)
    up = torch.randn(B, S, generator=g)
    zn = z.view(B, S, C).to(DEV).requires_grad_(True)
    rows = head(zn, labels.view(B, S).to(DEV), mask.view(B, S).to(DEV), "none")
    assert rows.shape == (B, S) and rows.requires_grad
    (rows * up.to(DEV)).sum().backward()
    zr = z.double().requires_grad_(True)
    r64 = T.row_values(zr, labels, live, weight, 0.1, 2.0)
    (g64,) = torch.autograd.grad((r64 * up.view(-1).double()).sum(), (zr,))
    value_close(rows.view(-1), r64.detach(), "rows")
    close(zn.grad.view(-1, C), g64, rtol=1e-4, name="dlogits (none)")
    # mean / sum and scale through the Function; [N,C]: B = 1
    for reduction in ("mean", "sum"):
        want, _, gw = T.ref_with_grads(z, labels, mask, weight, 0.1, 2.0, reduction, 1, 0.25)
        zq = z.to(DEV).requires_grad_(True)
        loss, rws, stats = engine.TokenCEFunction.apply(zq, labels.to(DEV), mask.to(DEV), weight.to(DEV), T.IGNORE, 0.1, 2.0,
                                                        reduction, 0.25)
        assert not rws.requires_grad and not stats.requires_grad
        (loss * T.UPSTREAM).backward()
        value_close(loss, want, reduction)
        close(zq.grad, gw, rtol=1e-4, name="dlogits " + reduction)
    # decode
    tags, logp = head.decode(z3.detach(), mask.view(B, S).to(DEV))
    assert tags.shape == (B, S) and tags.dtype == torch.int64 and logp.shape == (B, S)
    want = torch.where(mask.view(B, S) != 0, torch.argmax(z.view(B, S, C), -1), torch.zeros(B, S, dtype=torch.long))
    assert torch.equal(tags.cpu(), want)
    with pytest.raises(ValueError):
        head(z3, labels.view(B, S).to(DEV), None, "token_mean")
    with pytest.raises(ValueError):
        head(z3[..., :-1], labels.view(B, S).to(DEV))
    with pytest.raises(ValueError):
        engine.TokenCEFunction.apply(z3, labels.to(DEV))


def test_error_codes_come_back_before_any_launch(hip):
    lib = hip.lib()
    z = torch.zeros(4, 64, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.full((4 * 64 + 8,), 7.0, device=DEV)
    stats = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    tags = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()
    st = hip._st()

    def fwd(N=4, C=64, eps=0.0, gamma=0.0, red=0, B=1, logits=z, labels=lab, stats_=stats):
        return lib.mtvaf_token_ce_fwd(p(logits) if logits is not None else None, p(labels) if labels is not None else None, None,
                                      None, p(out), p(out[1:]), p(stats_) if stats_ is not None else None, N, C, T.IGNORE, eps,
                                      gamma, red, B, 1.0, st)

    def bwd(N=4, C=64, eps=0.0, gamma=0.0, red=0, B=1, logits=z, labels=lab, gout=True, grows=False):
        return lib.mtvaf_token_ce_bwd(p(out) if gout else None, p(out[1:]) if grows else None,
                                      p(logits) if logits is not None else None, p(labels) if labels is not None else None, None,
                                      None, p(out[8:]), N, C, T.IGNORE, eps, gamma, red, B, 1.0, st)

    for call in (fwd, bwd):
        assert call(C=0) == ERR_SHAPE and call(C=65) == ERR_SHAPE and call(N=0) == ERR_SHAPE
        assert call(eps=1.0) == ERR_ARG and call(eps=-0.1) == ERR_ARG and call(eps=float("nan")) == ERR_ARG
        assert call(gamma=0.5) == ERR_ARG and call(gamma=8.5) == ERR_ARG and call(gamma=-1.0) == ERR_ARG
        assert call(gamma=float("nan")) == ERR_ARG
        assert call(red=3) == ERR_ARG and call(red=-1) == ERR_ARG and call(red=1, B=0) == ERR_ARG
        assert call(logits=None) == ERR_ARG and call(labels=None) == ERR_ARG
    assert fwd(stats_=None) == ERR_ARG
    assert bwd(gout=False, grows=False) == ERR_ARG and bwd(gout=True, grows=True) == ERR_ARG   # exactly one upstream gradient
    am = lambda N=4, C=64, logits=z, tg=tags: lib.mtvaf_token_argmax(p(logits) if logits is not None else None, None, None,
                                                                     p(tg) if tg is not None else None, p(out), N, C, st)
    assert am(C=0) == ERR_SHAPE and am(C=65) == ERR_SHAPE and am(N=0) == ERR_SHAPE
    assert am(logits=None) == ERR_ARG and am(tg=None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7).all()) and bool((tags == 7).all())  # nothing ran
    assert fwd(C=1, N=4) == OK and bwd(C=1, N=4, gamma=8.0, red=1) == OK and am(C=1) == OK


def test_the_pair_replays_from_a_captured_graph(hip):
    N, C = 257, 11
    z, labels, mask, weight = T.make_logits(N, C), T.make_labels(N, C), T.make_mask("prefix", N), T.make_weights(C)
    eager = run_abi(hip, z, labels, mask, weight, 0.1, 2.0)
    zg, lg, mg, wg = z.to(DEV), labels.to(DEV), mask.to(DEV), weight.to(DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    loss, rows, dz, stats = nan(1), nan(N), nan(N, C), torch.zeros(2, dtype=torch.int32, device=DEV)
    up = torch.full((1,), T.UPSTREAM, device=DEV)
    how = (T.IGNORE, 0.1, 2.0, 0, 1, 1.0)
    torch.cuda.synchronize()  # (the eager call above loaded the library)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.token_ce_fwd(zg, lg, mg, wg, loss, rows, stats, *how)
        hip.token_ce_bwd(up, None, zg, lg, mg, wg, dz, *how)
    for _ in range(2):
        for t in (loss, rows, dz):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, (loss, rows, stats, dz)):
            assert torch.equal(a, b)
