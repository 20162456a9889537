"""The span-model heads of csrc/span.hip against the float64 references of span_cases.py (whose case tables and bounds
test_span_cases.py proves on the host), through the hip.* wrappers: every output of a call is a view into ONE flat allocation
with sentinel guards around it, every case asserts excess <= 1 (error / bound, the message carries the worst one), the index
block and mask_mul are compared bit for bit, and every forward and backward is repeated and must return the same bits."""
import ctypes
import math

import pytest
import torch

import span_cases as SC
from test_ln_kernels_gpu import Flat

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_ = SC.SENTINEL
ERR_SHAPE, ERR_WORKSPACE = -1, -4  # include/mtvaf_hip.h


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def cid(c):
    return c["id"]


def assert_within(tag, e):
    print(tag, {k: round(v, 4) for k, v in e.items()})
    worst = max(e, key=lambda k: e[k] if e[k] == e[k] else float("inf"))
    assert all(v <= 1 for v in e.values()), (tag, "worst excess", worst, e[worst], e)


# ---------------------------------------------------------------------------------------------------------------------
# span_index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.INDEX_CASES, ids=cid)
def test_span_index_whole_block(hip, c):
    mask, starts, ends = SC.index_inputs(c)
    want, spec = SC.index_ref(mask, starts, ends)
    m, s, e = mask.to(DEV), starts.to(DEV), ends.to(DEV)
    got = hip.span_index(m, s, e)
    assert got.numel() == want.numel() == hip.lib().mtvaf_span_index_ints(c["B"], c["S"], c["M"])
    bad = (got.cpu() != want) & spec
    assert not bool(bad.any()), (c["id"], bad.nonzero().view(-1)[:8].tolist())
    assert torch.equal(hip.span_index(m, s, e).cpu()[spec], got.cpu()[spec])


# ---------------------------------------------------------------------------------------------------------------------
# span pooling
# ---------------------------------------------------------------------------------------------------------------------
def pool_buffers(B, S, M, H):
    return Flat([("pooled", B * M * H), ("stats", 2 * B * M), ("dseq", B * S * H), ("dw", H), ("db", 1)])


def run_pool(hip, c):
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(c)
    B, S, M, H = c["B"], c["S"], c["M"], c["H"]
    index = hip.span_index(mask.to(DEV), starts.to(DEV), ends.to(DEV))
    d = [t.to(DEV).contiguous() for t in (seq, wu, bu, gw)]
    outs = []
    for _ in range(2):
        o = pool_buffers(B, S, M, H)
        hip.span_pool_fwd(d[0], d[1], d[2], index, o["pooled"], o["stats"], B, S, M)
        hip.span_pool_bwd(d[3], o["pooled"], o["stats"], d[0], d[1], d[2], index, o["dseq"], o["dw"], o["db"], B, S, M)
        assert o.intact(), c["id"]
        outs.append(o)
    assert torch.equal(outs[0].buf, outs[1].buf), c["id"]  # forward and backward repeat bit for bit
    o = outs[0]
    return (o["pooled"].cpu().view(B * M, H), o["dseq"].cpu().view(B * S, H), o["dw"].cpu(), o["db"].cpu()), o


@pytest.mark.parametrize("c", SC.POOL_CASES, ids=cid)
def test_span_pool_fwd_bwd(hip, c):
    inp = SC.pool_inputs(c)
    got, o = run_pool(hip, c)
    ref = SC.pool_ref(*inp)
    t = SC.pool_terms(*inp, cond=c["score"] in SC.POOL_COND_KINDS)
    assert not bool((o["stats"] == S_).any())
    assert_within(c["id"], {"pooled": SC.excess(got[0], ref[0], SC.RTOL_POOLED, t["pooled"]),
                            "dseq": SC.excess(got[1], ref[1], SC.RTOL_POOL_GRAD, t["dseq"]),
                            "dw": SC.excess(got[2], ref[2], SC.RTOL_POOL_GRAD, t["dw"]),
                            "db": SC.excess(got[3], ref[3], SC.RTOL_POOL_GRAD, t["db"])})
    dead = (inp[1].reshape(-1) == 0) | ~SC.rows_read(*inp[1:4])  # masked rows and rows no span reads: exactly nothing
    assert not bool(got[1][dead].any()), c["id"]


@pytest.mark.parametrize("c", SC.POOL_ZERO_CASES, ids=cid)
def test_span_pool_nothing_to_pool_is_exactly_zero(hip, c):
    got, o = run_pool(hip, c)
    for name, t in zip(("pooled", "dseq", "dw", "db"), got):
        assert not bool(t.any()), (c["id"], name)


@pytest.mark.parametrize("H", SC.POOL_REJECTED_H)
def test_span_pool_rejects_the_width(hip, H):
    B, S, M = 2, 6, 3
    seq, mask, starts, ends, _, bu, _ = SC.pool_inputs(SC.POOL_CASES[0])
    index = hip.span_index(mask.to(DEV), starts.to(DEV), ends.to(DEV))
    x, w, g = torch.zeros(B, S, H, device=DEV), torch.zeros(1, H, device=DEV), torch.zeros(B * M, H, device=DEV)
    o = pool_buffers(B, S, M, max(H, 4))
    with pytest.raises(RuntimeError, match="mtvaf_span_pool_fwd"):
        hip.span_pool_fwd(x, w, bu.to(DEV), index, o["pooled"], o["stats"], B, S, M)
    with pytest.raises(RuntimeError, match="mtvaf_span_pool_bwd"):
        hip.span_pool_bwd(g, o["pooled"], o["stats"], x, w, bu.to(DEV), index, o["dseq"], o["dw"], o["db"], B, S, M)
    P = hip._p
    assert hip.lib().mtvaf_span_pool_fwd(P(x), P(w), P(bu.to(DEV)), P(index), P(o["pooled"]), P(o["stats"]), B, S, M, H,
                                         hip._st()) == ERR_SHAPE
    assert o.untouched()


def test_span_pool_bwd_rejects_a_short_workspace(hip):
    c = SC.POOL_CASES[0]
    B, S, M, H = c["B"], c["S"], c["M"], c["H"]
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(c)
    index = hip.span_index(mask.to(DEV), starts.to(DEV), ends.to(DEV))
    d = [t.to(DEV).contiguous() for t in (seq, wu, bu, gw)]
    wsb = hip.lib().mtvaf_span_pool_bwd_workspace_bytes(B, S, M, H)
    assert wsb == (2 * B * M * S + B * M * H + B * M) * 4
    o = pool_buffers(B, S, M, H)
    ws = Flat([("ws", wsb // 4)])
    dwp, dbp = ctypes.c_void_p(), ctypes.c_void_p()
    P = hip._p
    rc = hip.lib().mtvaf_span_pool_bwd(P(d[3]), P(d[3]), P(o["stats"]), P(d[0]), P(d[1]), P(d[2]), P(index), P(o["dseq"]),
                                       ctypes.byref(dwp), ctypes.byref(dbp), B, S, M, H, P(ws["ws"]), wsb - 1, hip._st())
    assert rc == ERR_WORKSPACE and o.untouched() and ws.untouched() and dwp.value is None and dbp.value is None


# ---------------------------------------------------------------------------------------------------------------------
# distant cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def run_dce(hip, c):
    """-> loss, dlogits [B, S] (cpu); asserts the guards, the skipped columns and the repeat"""
    B, S, ld, ldd = c["B"], c["S"], c["ld"], c["ldd"]
    z, pos = SC.dce_inputs(c)
    zs = torch.full((B * S, ld), float("nan"))  # the columns a call must not read
    zs[:, 0] = z.reshape(-1)
    zd, pd = zs.to(DEV), pos.to(DEV).contiguous()
    gout = torch.tensor([c["gout"]], device=DEV)
    outs = []
    for _ in range(2):
        o = Flat([("loss", 1), ("row_ws", 3 * B), ("dlogits", B * S * ldd)])
        o["loss"].fill_(SC.DCE_PRIOR if c["acc"] else float("nan"))
        hip.distant_ce_fwd(zd, ld, pd, o["loss"], o["row_ws"], B, S, c["scale"], c["acc"])
        hip.distant_ce_bwd(gout, c["scale"], zd, ld, pd, o["row_ws"], o["dlogits"], ldd, B, S)
        assert o.intact(), c["id"]
        outs.append(o)
    a, b = outs[0].buf.cpu(), outs[1].buf.cpu()
    assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)), c["id"]
    dl = outs[0]["dlogits"].cpu().view(B * S, ldd)
    assert bool((dl[:, 1:] == S_).all()), c["id"]  # the columns between the strided elements stay as they were
    return float(outs[0]["loss"].cpu()), dl[:, 0].reshape(B, S)


@pytest.mark.parametrize("c", SC.DCE_CASES, ids=cid)
def test_distant_ce_fwd_bwd(hip, c):
    z, pos = SC.dce_inputs(c)
    rl, rd = SC.dce_ref(z, pos, c["scale"], c["gout"])
    loss, dl = run_dce(hip, c)
    want = float(rl) + (SC.DCE_PRIOR if c["acc"] else 0.0)
    assert_within(c["id"], {"loss": SC.loss_excess(loss, want), "dlogits": SC.excess(dl, rd, SC.RTOL_DLOGITS)})


def test_distant_ce_row_without_a_position_is_nan_like_the_reference(hip):
    c = SC.DCE_EMPTY_ROW_CASE
    z, pos = SC.dce_inputs(c)
    rl, rd = SC.dce_ref(z, pos, c["scale"], c["gout"])
    loss, dl = run_dce(hip, c)
    r = c["empty_row"]
    live = [b for b in range(c["B"]) if b != r]
    assert math.isnan(float(rl)) and math.isnan(loss) and bool(dl[r].isnan().all())
    assert_within(c["id"], {"dlogits": SC.excess(dl[live], rd[live], SC.RTOL_DLOGITS)})


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def run_ce(hip, c):
    N, C = c["N"], c["C"]
    z, lab = SC.ce_inputs(c)
    zd, ld_ = z.to(DEV).contiguous(), lab.to(DEV)
    gout = torch.tensor([SC.CE_GOUT], device=DEV)
    outs = []
    for _ in range(2):
        o = Flat([("loss", 1), ("ws2", 2), ("dlogits", N * C)])
        hip.ce_fwd(zd, ld_, o["loss"], o["ws2"])
        hip.ce_bwd(gout, zd, ld_, o["ws2"], o["dlogits"])
        assert o.intact(), c["id"]
        outs.append(o)
    a, b = outs[0].buf.cpu(), outs[1].buf.cpu()
    assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)), c["id"]
    o = outs[0]
    return float(o["loss"].cpu()), o["ws2"].cpu(), o["dlogits"].cpu().view(N, C)


@pytest.mark.parametrize("c", SC.CE_CASES, ids=cid)
def test_ce_fwd_bwd(hip, c):
    z, lab = SC.ce_inputs(c)
    rl, rd, rt, cnt = SC.ce_ref(z, lab)
    loss, ws2, dl = run_ce(hip, c)
    assert float(ws2[1]) == cnt
    assert_within(c["id"], {"loss": SC.loss_excess(loss, rl, SC.ce_sum_term(cnt, rl)),
                            "ws2": SC.loss_excess(ws2[0], rt, SC.ce_sum_term(cnt, rt)),
                            "dlogits": SC.excess(dl, rd, SC.RTOL_DLOGITS)})
    assert not bool(dl[lab == -100].any()), c["id"]


def test_ce_no_row_counted(hip):
    c = SC.CE_ALL_IGNORED_CASE
    rl = SC.ce_ref(*SC.ce_inputs(c))[0]
    loss, ws2, dl = run_ce(hip, c)
    assert math.isnan(float(rl)) and math.isnan(loss)  # 0 / 0, as torch
    assert ws2.tolist() == [0.0, 0.0] and not bool(dl.any())


@pytest.mark.parametrize("C", SC.CE_REJECTED_C)
def test_ce_rejects_the_class_count(hip, C):
    N = 3
    z, lab = torch.zeros(N, C, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV)
    o = Flat([("loss", 1), ("ws2", 2), ("dlogits", N * max(C, 1))])
    with pytest.raises(RuntimeError, match="mtvaf_ce_fwd"):
        hip.ce_fwd(z, lab, o["loss"], o["ws2"])
    with pytest.raises(RuntimeError, match="mtvaf_ce_bwd"):
        hip.ce_bwd(torch.ones(1, device=DEV), z, lab, o["ws2"], o["dlogits"])
    assert o.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# mask_mul
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,which", [(s, w) for s in SC.MASK_MUL_SHAPES for w in SC.MASK_MUL_KEEPS],
                         ids=lambda v: SC.MASK_MUL_SHAPES.get(v, v) if isinstance(v, tuple) else v)
def test_mask_mul_is_two_rounded_products(hip, shape, which):
    B, S, H = shape
    x, row, col = SC.mask_mul_inputs(B, S, H, which)
    want = SC.mask_mul_ref(x, row, col)
    xd = x.to(DEV)
    rd, cd = (t.to(DEV).contiguous() if t is not None else None for t in (row, col))
    o = Flat([("out", x.numel())])
    hip.mask_mul(xd, rd, cd, o["out"])
    assert o.intact(), SC.mask_mul_id(shape, which)
    got = o["out"].cpu().view(B, S, H)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), SC.mask_mul_id(shape, which)
    o2 = Flat([("out", x.numel())])
    hip.mask_mul(xd, rd, cd, o2["out"])
    assert torch.equal(o2["out"], o["out"])


def test_mask_mul_rejects_the_width(hip):
    H = SC.MASK_MUL_REJECTED_H
    o = Flat([("out", 2 * H)])
    with pytest.raises(RuntimeError, match="mtvaf_mask_mul"):
        hip.mask_mul(torch.zeros(1, 2, H, device=DEV), None, None, o["out"])
    assert o.untouched()
