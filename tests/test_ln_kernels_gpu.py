"""The LayerNorm and embedding row kernels of csrc/rowops.hip against the float64 references of ln_cases.py (whose case tables and
bounds test_ln_cases.py proves on the host), through the C ABI: every output of a call is a view into ONE flat allocation with
sentinel guards around it, every forward case compares mean and rstd, integer and bf16 results are compared bit for bit, and the
backward runs under both settings of MTVAF_LN_LEAN wherever the lean kernel's shape rule holds.

MODE 1 (embeddings) applies dropout BEHIND the LayerNorm: its dz has no zero pattern (the row means spread every kept gradient
over the row), so "exact zero where dropped" is asserted on the forward output there and on dx of MODE 0."""
import os

import pytest
import torch

import ln_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_ = LC.SENTINEL
OK, ERR_SHAPE, ERR_ARG, ERR_WORKSPACE = 0, -1, -3, -4  # include/mtvaf_hip.h
SEED, OFFSET = 77, 5


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


class Flat:
    """one allocation filled with the sentinel; named fp32 views [(name, floats)] (a (name, floats, shift) entry starts `shift`
    floats off the 16-byte grid)"""

    def __init__(self, spec):
        spec = [(s + (0,))[:3] for s in spec]
        sizes = [(n, sh) for _, n, sh in spec]
        offs, total = LC.view_layout(sizes)
        self.buf = torch.full((total,), S_, device=DEV)
        self.guard = LC.guard_mask(total, offs, [n for n, _ in sizes])
        self.v = {name: self.buf[o:o + n] for (name, n, _), o in zip(spec, offs)}

    def __getitem__(self, name):
        return self.v[name]

    def intact(self):
        return bool((self.buf.cpu()[self.guard] == S_).all())

    def untouched(self):
        return bool((self.buf == S_).all())


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bf16_copy(view, fp32):
    """the bf16 copy inside an fp32 view equals fp32.to(bfloat16) bit for bit"""
    return torch.equal(bits16(view.view(torch.bfloat16).cpu()), bits16(fp32.cpu().reshape(-1).to(torch.bfloat16)))


_keeps = {}


def device_keep(hip, M, H, p, seed=SEED, offset=OFFSET):
    """hip.dropout(ones) at the same (seed, offset): 0 or float32(1 / (1 - p)) per element -> cpu fp32 [M, H] (None at p = 0)"""
    if p <= 0:
        return None
    key = (M, H, p, seed, offset)
    if key not in _keeps:
        out = torch.empty(M * H, device=DEV)
        hip.dropout(torch.ones(M * H, device=DEV), out, p, seed, offset)
        _keeps[key] = out.cpu().view(M, H)
    return _keeps[key]


class lean_setting:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        if self.value is not None:
            os.environ["MTVAF_LN_LEAN"] = self.value

    def __exit__(self, *a):
        os.environ.pop("MTVAF_LN_LEAN", None)


def lean_settings(H):
    """the backward kernels a shape can take: unset (lean where its rule holds) and, there, MTVAF_LN_LEAN=0 (wave per row)"""
    return [None, "0"] if LC.lean_shape(H) else [None]


def dev(*ts):
    return [t.to(DEV).contiguous() if t is not None else None for t in ts]


def check_fwd(tag, o, M, H, ref, z, cond=None):
    ry, rmean, rstd = ref
    e = {"y": LC.excess(o["out"].view(M, H), ry, LC.RTOL_ROW, cond["y"] if cond else None),
         "mean": LC.mean_excess(o["mean"], rmean, z), "rstd": LC.rstd_excess(o["rstd"], rstd, z)}
    print(tag, "fwd", {k: round(v, 4) for k, v in e.items()})
    for k, v in e.items():
        assert v <= 1, (tag, k, v)


def check_bwd(tag, got, ref, keep, cond=None, prev=None):
    """got: dict of cpu tensors dx (or None), dres, dgamma, dbeta, dbias_x (or None); ref: res_ln_bwd_ref's tuple; prev: what the
    accumulating outputs held before (dres, dgamma, dbeta, dbias_x)"""
    names = ("dx", "dres", "dgamma", "dbeta", "dbias_x")
    e = {}
    for i, n in enumerate(names):
        if got.get(n) is None:
            continue
        r = ref[i] + (prev[n].double() if prev and n in prev else 0)
        extra = cond.get("dx" if n in ("dx", "dres") else n) if cond else None
        e[n] = LC.excess(got[n].view(r.shape), r, LC.RTOL_ROW if i < 2 else LC.RTOL_COL, extra)
    print(tag, "bwd", {k: round(v, 4) for k, v in e.items()})
    for k, v in e.items():
        assert v <= 1, (tag, k, v)
    if keep is not None and got.get("dx") is not None:  # exactly nothing where the element was dropped
        assert not bool(got["dx"].view(keep.shape)[keep == 0].any()), tag


def res_ln_fwd(hip, x, res, gamma, beta, eps, p, bf16=True):
    M, H = x.shape
    o = Flat([("out", M * H), ("mean", M), ("rstd", M), ("out16", M * H // 2)])
    gx, gr, gg, gb = dev(x, res, gamma, beta)
    P = hip._p
    rc = hip.lib().mtvaf_dropout_res_ln_fwd(P(gx), P(gr), P(gg), P(gb), P(o["out"]), P(o["mean"]), P(o["rstd"]), M, H, eps, p, SEED, OFFSET,
                                            P(o["out16"]) if bf16 else None, hip._st())
    assert rc == OK and o.intact()
    if bf16:
        assert same_bf16_copy(o["out16"], o["out"])
    else:
        assert bool((o["out16"] == S_).all())
    return o


def res_ln_bwd(hip, dout, x, res, gamma, mean, rstd, p, split, dres_acc, acc, with_dbias, dx_fp32, dx_bf16, prev=None):
    """mtvaf_dropout_res_ln_bwd (split False) or _bwd_rows + _bwd_finish (split True) -> (Flat, dict of cpu results)"""
    M, H = x.shape
    L = hip.lib()
    nb = int(L.mtvaf_ln_bwd_workspace_bytes(M, H))
    o = Flat([("dx", M * H), ("dres", M * H), ("dgamma", H), ("dbeta", H), ("dbias_x", H), ("dx16", M * H // 2), ("part", nb // 4)])
    if prev:
        for k, t in prev.items():
            o[k].copy_(t.reshape(-1))
    gd, gx, gr, gg = dev(dout, x, res, gamma)
    P = hip._p
    pdx, p16, pdb = (P(o["dx"]) if dx_fp32 else None), (P(o["dx16"]) if dx_bf16 else None), (P(o["dbias_x"]) if with_dbias else None)
    if split:
        rc = L.mtvaf_dropout_res_ln_bwd_rows(P(gd), P(gx), P(gr), P(gg), P(mean), P(rstd), pdx, P(o["dres"]), dres_acc, M, H, p, SEED, OFFSET,
                                             P(o["part"]), p16, hip._st())
        assert rc == OK
        rc = L.mtvaf_dropout_res_ln_bwd_finish(P(o["part"]), M, H, P(o["dgamma"]), P(o["dbeta"]), pdb, acc, hip._st())
    else:
        rc = L.mtvaf_dropout_res_ln_bwd(P(gd), P(gx), P(gr), P(gg), P(mean), P(rstd), pdx, P(o["dres"]), dres_acc, P(o["dgamma"]),
                                        P(o["dbeta"]), pdb, acc, M, H, p, SEED, OFFSET, P(o["part"]), nb, p16, hip._st())
    assert rc == OK and o.intact()
    got = {k: o[k].cpu() for k in ("dres", "dgamma", "dbeta")}
    got["dx"] = o["dx"].cpu() if dx_fp32 else None
    got["dbias_x"] = o["dbias_x"].cpu() if with_dbias else None
    if not dx_fp32:
        assert bool((o["dx"] == S_).all())
    if not with_dbias:
        assert bool((o["dbias_x"] == S_).all())
    if not dx_bf16:
        assert bool((o["dx16"] == S_).all())
    return o, got


def accumulate_prev(M, H):
    g = LC.gen(M + 3 * H)
    return {"dres": torch.randn(M, H, generator=g), "dgamma": torch.randn(H, generator=g), "dbeta": torch.randn(H, generator=g)}


def run_res_ln_case(hip, tag, x, res, gamma, beta, dout, eps, p, cond_kind=False):
    """forward, then under every backward kernel the shape can take: the one-call backward (overwriting, dbias_x, fp32 dx + bf16
    copy) and the split backward (accumulating dres / dgamma / dbeta, no dbias_x, dx = NULL with the bf16 copy alone)"""
    M, H = x.shape
    keep = device_keep(hip, M, H, p)
    ry, rmean, rstd, z = LC.res_ln_ref(x, res, gamma, beta, eps, keep)
    cond = LC.cond_terms(z, rstd, gamma, dout, keep) if cond_kind else None
    o = res_ln_fwd(hip, x, res, gamma, beta, eps, p)
    check_fwd(tag, o, M, H, (ry, rmean, rstd), z, cond)
    ref = LC.res_ln_bwd_ref(dout, x, res, gamma, eps, keep)
    prev = accumulate_prev(M, H)
    for lean in lean_settings(H):
        with lean_setting(lean):
            b, got = res_ln_bwd(hip, dout, x, res, gamma, o["mean"], o["rstd"], p, False, 0, 0, True, True, True)
            check_bwd("%s lean=%s one-call" % (tag, lean), got, ref, keep, cond)
            assert same_bf16_copy(b["dx16"], b["dx"])
            b2, got2 = res_ln_bwd(hip, dout, x, res, gamma, o["mean"], o["rstd"], p, True, 1, 1, False, False, True, prev)
            check_bwd("%s lean=%s rows+finish accumulating" % (tag, lean), got2, ref, keep, cond, prev)
            assert same_bf16_copy(b2["dx16"], b["dx"])  # dx = NULL: the bf16 copy alone, of the same values
    return o


# ---------------------------------------------------------------------------------------------------------------------
# residual LayerNorm: shapes, input kinds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.LN_SHAPES, ids=[LC.ln_shape_id(c) for c in LC.LN_SHAPES])
def test_res_ln_shapes(hip, case):
    M, H, _ = case
    x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, "unit")
    run_res_ln_case(hip, LC.ln_shape_id(case), x, res, gamma, beta, dout, eps, LC.LN_P)


@pytest.mark.parametrize("shape", LC.KIND_SHAPES, ids=["M%d-H%d" % s for s in LC.KIND_SHAPES])
@pytest.mark.parametrize("kind", LC.LN_KINDS)
def test_res_ln_input_kinds(hip, kind, shape):
    M, H = shape
    x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, kind)
    o = run_res_ln_case(hip, "%s M%d H%d" % (kind, M, H), x, res, gamma, beta, dout, eps, 0.0, kind in LC.COND_KINDS)
    if kind == "constant-row":  # sums of these constants are exact in fp32: the variance is exactly 0 and y is beta
        assert torch.equal(o["out"].cpu().view(M, H), beta.expand(M, H))
        assert torch.equal(o["mean"].cpu(), (x + res)[:, 0])
    if kind == "gamma0-beta1":
        assert bool((o["out"] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# residual LayerNorm: the slab and plane entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["no-bias", "bias"])
@pytest.mark.parametrize("nslab", LC.SLAB_COUNTS)
@pytest.mark.parametrize("shape", LC.VARIANT_SHAPES, ids=["M%d-H%d" % s for s in LC.VARIANT_SHAPES])
def test_res_ln_fwd_slabs(hip, shape, nslab, with_bias):
    M, H = shape
    _, res, gamma, beta, _, eps = LC.ln_inputs(M, H, "unit")
    slabs, bias = LC.slab_inputs(M, H, nslab)
    bias = bias if with_bias else None
    x32 = LC.slab_sum(slabs, bias, torch.float32)  # the kernel's order: the same bits
    keep = device_keep(hip, M, H, LC.LN_P)
    ry, rmean, rstd, z = LC.res_ln_ref(LC.slab_sum(slabs, bias), res, gamma, beta, eps, keep)
    o = Flat([("out", M * H), ("mean", M), ("rstd", M), ("x_out", M * H), ("out16", M * H // 2)])
    gs, gbias, gr, gg, gb = dev(slabs, bias, res, gamma, beta)
    P = hip._p
    rc = hip.lib().mtvaf_dropout_res_ln_fwd_slabs(P(gs), nslab, P(gbias), P(o["x_out"]), P(gr), P(gg), P(gb), P(o["out"]), P(o["mean"]),
                                                  P(o["rstd"]), M, H, eps, LC.LN_P, SEED, OFFSET, P(o["out16"]), hip._st())
    assert rc == OK and o.intact()
    assert torch.equal(o["x_out"].cpu().view(M, H), x32)
    check_fwd("slabs M%d H%d nslab%d" % (M, H, nslab), o, M, H, (ry, rmean, rstd), z)
    assert same_bf16_copy(o["out16"], o["out"])


@pytest.mark.parametrize("nslab", [0, 2])
@pytest.mark.parametrize("shape", LC.PLANE_SHAPES, ids=["M%d-H%d" % s for s in LC.PLANE_SHAPES])
def test_res_ln_fwd_planes(hip, shape, nslab):
    M, H = shape
    x, res, gamma, beta, _, eps = LC.ln_inputs(M, H, "unit")
    slabs, bias = LC.slab_inputs(M, H, max(nslab, 1))
    keep = device_keep(hip, M, H, LC.LN_P)
    xin = LC.slab_sum(slabs, bias) if nslab else x
    ry, rmean, rstd, z = LC.res_ln_ref(xin, res, gamma, beta, eps, keep)
    o = Flat([("out", M * H), ("mean", M), ("rstd", M), ("x_out", M * H), ("img", 3 * M * H // 2)])
    gx, gs, gbias, gr, gg, gb = dev(x, slabs, bias, res, gamma, beta)
    P = hip._p
    rc = hip.lib().mtvaf_dropout_res_ln_fwd_planes(P(gs if nslab else gx), nslab, P(gbias), P(o["x_out"]), P(gr), P(gg), P(gb), P(o["out"]),
                                                   P(o["mean"]), P(o["rstd"]), M, H, eps, LC.LN_P, SEED, OFFSET, P(o["img"]), hip._st())
    assert rc == OK and o.intact()
    check_fwd("planes M%d H%d nslab%d" % (M, H, nslab), o, M, H, (ry, rmean, rstd), z)
    if nslab:
        assert torch.equal(o["x_out"].cpu().view(M, H), LC.slab_sum(slabs, bias, torch.float32))
    else:
        assert bool((o["x_out"] == S_).all())
    want = hip.Planes(o["out"].view(M, H).clone(), True).img  # the image a split pass over the fp32 result writes
    assert torch.equal(bits16(o["img"].view(torch.bfloat16)), bits16(want))


def bwd_rows_variant(hip, entry, shape, nslab, lean, dres_acc, dx_fp32):
    """mtvaf_dropout_res_ln_bwd_rows_slabs / _rows_planes + _finish against the reference with dout = slabs + dout_base"""
    M, H = shape
    L = hip.lib()
    x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, "unit")
    slabs, _ = LC.slab_inputs(M, H, max(nslab, 1), seed=3)
    keep = device_keep(hip, M, H, LC.LN_P)
    f = res_ln_fwd(hip, x, res, gamma, beta, eps, LC.LN_P, bf16=False)
    dsum = LC.slab_sum(slabs) + dout.double() if nslab else dout.double()
    ref = LC.res_ln_bwd_ref(dsum, x, res, gamma, eps, keep)
    nb = int(L.mtvaf_ln_bwd_workspace_bytes(M, H))
    planes = entry == "planes"
    o = Flat([("dx", M * H), ("dres", M * H), ("dgamma", H), ("dbeta", H), ("dbias_x", H), ("dx16", 3 * M * H // 2 if planes else M * H // 2),
              ("part", nb // 4)])
    prev = accumulate_prev(M, H) if dres_acc else None
    if prev:
        o["dres"].copy_(prev["dres"].reshape(-1))
    gd, gs, gx, gr, gg = dev(dout, slabs, x, res, gamma)
    P = hip._p
    with lean_setting(lean):
        fn = L.mtvaf_dropout_res_ln_bwd_rows_planes if planes else L.mtvaf_dropout_res_ln_bwd_rows_slabs
        rc = fn(P(gd), P(gs) if nslab else None, nslab, P(gx), P(gr), P(gg), P(f["mean"]), P(f["rstd"]), P(o["dx"]) if dx_fp32 else None,
                P(o["dres"]), dres_acc, M, H, LC.LN_P, SEED, OFFSET, P(o["part"]), P(o["dx16"]), hip._st())
        assert rc == OK
        rc = L.mtvaf_dropout_res_ln_bwd_finish(P(o["part"]), M, H, P(o["dgamma"]), P(o["dbeta"]), P(o["dbias_x"]), 0, hip._st())
        assert rc == OK and o.intact()
        got = {k: o[k].cpu() for k in ("dres", "dgamma", "dbeta", "dbias_x")}
        got["dx"] = o["dx"].cpu() if dx_fp32 else None
        check_bwd("%s M%d H%d nslab%d lean=%s" % (entry, M, H, nslab, lean), got, ref, keep, None, {"dres": prev["dres"]} if prev else None)
        # the fp32 dx of the same kernel, for the copy / image of a call that wrote none
        if dx_fp32:
            dx = o["dx"].view(M, H).clone()
        else:
            assert bool((o["dx"] == S_).all())
            o2 = Flat([("dx", M * H), ("dres", M * H), ("dx16", 3 * M * H // 2), ("part", nb // 4)])
            rc = fn(P(gd), P(gs) if nslab else None, nslab, P(gx), P(gr), P(gg), P(f["mean"]), P(f["rstd"]), P(o2["dx"]), P(o2["dres"]), 0,
                    M, H, LC.LN_P, SEED, OFFSET, P(o2["part"]), P(o2["dx16"]), hip._st())
            assert rc == OK and o2.intact()
            dx = o2["dx"].view(M, H).clone()
    if planes:
        assert torch.equal(bits16(o["dx16"].view(torch.bfloat16)), bits16(hip.Planes(dx, True).img))
    else:
        assert same_bf16_copy(o["dx16"], dx)


@pytest.mark.parametrize("lean", [None, "0"], ids=["lean-where-it-applies", "wave-per-row"])
@pytest.mark.parametrize("nslab", LC.SLAB_COUNTS)
@pytest.mark.parametrize("shape", LC.VARIANT_SHAPES, ids=["M%d-H%d" % s for s in LC.VARIANT_SHAPES])
def test_res_ln_bwd_rows_slabs(hip, shape, nslab, lean):
    bwd_rows_variant(hip, "slabs", shape, nslab, lean, dres_acc=nslab % 2, dx_fp32=nslab != 2)


@pytest.mark.parametrize("lean", [None, "0"], ids=["lean-where-it-applies", "wave-per-row"])
@pytest.mark.parametrize("nslab", [0, 2])
@pytest.mark.parametrize("shape", LC.PLANE_SHAPES, ids=["M%d-H%d" % s for s in LC.PLANE_SHAPES])
def test_res_ln_bwd_rows_planes(hip, shape, nslab, lean):
    bwd_rows_variant(hip, "planes", shape, nslab, lean, dres_acc=1 if nslab else 0, dx_fp32=nslab == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the exact cross-kernel contract of the keep factor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LC.EXACT_SHAPES, ids=["M%d-H%d" % s for s in LC.EXACT_SHAPES])
@pytest.mark.parametrize("p", LC.EXACT_PS)
def test_every_dropout_site_scales_as_mtvaf_dropout_bit_for_bit(hip, p, shape):
    """embed_ln_fwd with gamma = 0, beta = 1 writes dropout(1); the MODE 0 backward on exact_bwd_inputs writes +-keep: both must be
    hip.dropout(ones, p, seed, offset) bit for bit (at p = 0.9: 10, where 1.f / (1.f - p) in fp32 gave 9.999998)."""
    M, H = shape
    seed, off = LC.EXACT_SEED, LC.EXACT_OFFSET
    mask = device_keep(hip, M, H, p, seed, off)
    vals = set(mask.unique().tolist())
    assert vals <= {0.0, float(LC.dropout_scale(p))} and (M * H < 1000 or len(vals) == 2)
    L, P = hip.lib(), hip._p
    # MODE 1
    o = Flat([("out", M * H), ("mean", M), ("rstd", M)])
    ids, tts = torch.zeros(1, M, dtype=torch.int64, device=DEV), torch.zeros(1, M, dtype=torch.int64, device=DEV)
    g = LC.gen(H)
    word, pos, typ = dev(torch.randn(2, H, generator=g), torch.randn(M, H, generator=g), torch.randn(1, H, generator=g))
    gamma, beta = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
    rc = L.mtvaf_embed_ln_fwd(P(ids), P(tts), None, P(word), P(pos), P(typ), P(gamma), P(beta), P(o["out"]), P(o["mean"]), P(o["rstd"]), 1, M,
                              H, 1e-12, p, seed, off, None, hip._st())
    assert rc == OK and o.intact()
    assert torch.equal(o["out"].cpu().view(M, H).view(torch.int32), mask.view(torch.int32))
    # MODE 0 backward, both kernels
    x, res, gam, mean, rstd, dout = LC.exact_bwd_inputs(M, H)
    nb = int(L.mtvaf_ln_bwd_workspace_bytes(M, H))
    gx, gr, gg, gm, gs, gd = dev(x, res, gam, mean, rstd, dout)
    for lean in lean_settings(H):
        with lean_setting(lean):
            b = Flat([("dx", M * H), ("dres", M * H), ("part", nb // 4)])
            rc = L.mtvaf_dropout_res_ln_bwd_rows(P(gd), P(gx), P(gr), P(gg), P(gm), P(gs), P(b["dx"]), P(b["dres"]), 0, M, H, p, seed, off,
                                                 P(b["part"]), None, hip._st())
            assert rc == OK and b.intact()
            dx = b["dx"].cpu().view(M, H)
            assert torch.equal(dx == 0, mask == 0), lean  # the zero pattern is the mask
            assert torch.equal(dx.abs().view(torch.int32), mask.view(torch.int32)), lean
            assert torch.equal(b["dres"].cpu().view(M, H), dout)


# ---------------------------------------------------------------------------------------------------------------------
# embeddings
# ---------------------------------------------------------------------------------------------------------------------
def run_embed(hip, c, check=True):
    """embed_ln_fwd + embed_ln_bwd of a case -> (dict of cpu results, the case's inputs, the reference tuple)"""
    e = LC.embed_inputs(c)
    B, S, H, vocab, max_pos, tv, p = e["B"], e["S"], c["H"], c["vocab"], e["max_pos"], c["type_vocab"], c["p"]
    M = B * S
    L, P = hip.lib(), hip._p
    keep = device_keep(hip, M, H, p, LC.EMBED_SEED, LC.EMBED_OFFSET)
    ids, tts, pos_ids, word, pos, typ, gamma, beta, dout = dev(e["ids"], e["tts"], e["pos_ids"], e["word"], e["pos"], e["typ"], e["gamma"],
                                                               e["beta"], e["dout"])
    a = (e["ids"], e["tts"], e["pos_ids"], e["word"], e["pos"], e["typ"], e["gamma"])
    f = Flat([("out", M * H), ("mean", M), ("rstd", M), ("out16", M * H // 2)])
    rc = L.mtvaf_embed_ln_fwd(P(ids), P(tts), P(pos_ids), P(word), P(pos), P(typ), P(gamma), P(beta), P(f["out"]), P(f["mean"]), P(f["rstd"]),
                              B, S, H, e["eps"], p, LC.EMBED_SEED, LC.EMBED_OFFSET, P(f["out16"]), hip._st())
    assert rc == OK and f.intact()
    r_out, r_mean, r_rstd, z = LC.embed_ln_ref(*a, e["beta"], e["eps"], keep)
    if check:
        check_fwd(c["id"], f, M, H, (r_out, r_mean, r_rstd), z)
        assert same_bf16_copy(f["out16"], f["out"])
        if keep is not None:
            assert not bool(f["out"].cpu().view(M, H)[keep == 0].any())
    wsb = int(L.mtvaf_embed_ln_bwd_workspace_bytes(M, H, vocab, max_pos))
    b = Flat([("dword", vocab * H), ("dpos", max_pos * H), ("dtype", tv * H), ("dgamma", H), ("dbeta", H), ("dz", M * H),
              ("ws", (wsb + 3) // 4)])
    for k, t in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), e["prev"]):
        b[k].copy_(t.reshape(-1))
    rc = L.mtvaf_embed_ln_bwd(P(dout), P(ids), P(tts), P(pos_ids), P(word), P(pos), P(typ), P(gamma), P(f["mean"]), P(f["rstd"]), P(b["dword"]),
                              P(b["dpos"]), P(b["dtype"]), P(b["dgamma"]), P(b["dbeta"]), c["acc"], B, S, H, vocab, max_pos, tv, e["word_pad"],
                              e["pos_pad"], p, LC.EMBED_SEED, LC.EMBED_OFFSET, P(b["dz"]), P(b["ws"]), wsb, hip._st())
    assert rc == OK and b.intact()
    got = {k: b[k].cpu() for k in ("dz", "dword", "dpos", "dtype", "dgamma", "dbeta")}
    ref = LC.embed_ln_bwd_ref(e["dout"], *a, e["eps"], e["word_pad"], e["pos_pad"], keep, e["prev"] if c["acc"] else None)
    if check:
        ex = {}
        for i, k in enumerate(("dz", "dword", "dpos", "dtype", "dgamma", "dbeta")):
            ex[k] = LC.excess(got[k].view(ref[i].shape), ref[i], LC.RTOL_ROW if i == 0 else LC.RTOL_COL)
        print(c["id"], "bwd", {k: round(v, 4) for k, v in ex.items()})
        for k, v in ex.items():
            assert v <= 1, (c["id"], k, v)
        # table rows no token names: exactly zero when overwriting, exactly what they held when accumulating
        used_w = torch.zeros(vocab, dtype=torch.bool)
        used_w[e["ids"].reshape(-1)[e["ids"].reshape(-1) != e["word_pad"]]] = True
        used_p = torch.zeros(max_pos, dtype=torch.bool)
        if e["pos_ids"] is None:
            used_p[:S] = True
        else:
            fp = e["pos_ids"].reshape(-1).long()
            used_p[fp[fp != e["pos_pad"]]] = True
        for k, used, prev in (("dword", used_w, e["prev"][0]), ("dpos", used_p, e["prev"][1])):
            rest = got[k].view(prev.shape)[~used]
            assert torch.equal(rest, prev[~used] if c["acc"] else torch.zeros_like(rest)), (c["id"], k)
    return got, e, ref


@pytest.mark.parametrize("case", LC.EMBED_CASES, ids=[c["id"] for c in LC.EMBED_CASES])
def test_embed_ln(hip, case):
    run_embed(hip, case)


def test_embed_ln_vocab_above_the_scan_limit_takes_the_atomic_scatter(hip):
    run_embed(hip, LC.EMBED_ATOMIC_CASE)  # (tolerance only: float atomics)


def test_embed_ln_deterministic_scatter_twice_gives_the_same_bits(hip):
    a, _, _ = run_embed(hip, LC.EMBED_TWICE_CASE)
    b, _, _ = run_embed(hip, LC.EMBED_TWICE_CASE, check=False)
    assert torch.equal(a["dword"], b["dword"]) and torch.equal(a["dpos"], b["dpos"])


def test_embed_ln_atomic_scatter_mode_against_the_deterministic_one(hip):
    L = hip.lib()
    before = L.mtvaf_embed_scatter_mode(-1)
    try:
        assert L.mtvaf_embed_scatter_mode(0) == 0
        det, _, _ = run_embed(hip, LC.EMBED_MODE_CASE)
        assert L.mtvaf_embed_scatter_mode(1) == 1
        ato, _, ref = run_embed(hip, LC.EMBED_MODE_CASE)  # (checked against float64 at the same bounds)
        assert LC.excess(ato["dword"].view(ref[1].shape), det["dword"].view(ref[1].shape).double(), LC.RTOL_COL) <= 1
    finally:
        L.mtvaf_embed_scatter_mode(before)
    assert L.mtvaf_embed_scatter_mode(-1) == before


# ---------------------------------------------------------------------------------------------------------------------
# RoBERTa position ids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", LC.POS_S)
def test_roberta_position_ids(hip, S):
    ids = LC.pos_ids_inputs(S)
    B = ids.shape[0]
    out = torch.full((B * S + 16,), -7, dtype=torch.int32, device=DEV)
    gi = ids.to(DEV)
    rc = hip.lib().mtvaf_roberta_position_ids(hip._p(gi), hip._p(out[8:]), B, S, LC.POS_PAD, hip._st())
    assert rc == OK
    got = out.cpu()
    assert torch.equal(got[8:8 + B * S].view(B, S).long(), LC.roberta_pos_ref(ids, LC.POS_PAD))
    assert bool((got[:8] == -7).all()) and bool((got[8 + B * S:] == -7).all())


# ---------------------------------------------------------------------------------------------------------------------
# rejections: the documented error, nothing written
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_return_the_documented_error_and_write_nothing(hip):
    L, P = hip.lib(), hip._p
    st = hip._st()
    M, H = 4, 32
    o = Flat([("out", 2 * M * 1028), ("mean", M), ("rstd", M), ("x_out", M * 1028), ("img", 3 * M * 1028 // 2), ("dx", M * 1028),
              ("dres", M * 1028), ("dgamma", 1028), ("dbeta", 1028), ("dbias_x", 1028), ("part", 4 * 4 * 1028), ("misaligned", 3 * M * H // 2, 1),
              ("dword", 16 * 1028), ("dpos", 16 * 1028), ("dtype", 3 * 1028), ("dz", M * 1028), ("ws", 1 << 16)])
    src = torch.ones(3 * M * 1028, device=DEV)
    ids = torch.zeros(1, M, dtype=torch.int64, device=DEV)
    s = P(src)
    fwd = lambda m, h: L.mtvaf_dropout_res_ln_fwd(s, s, s, s, P(o["out"]), P(o["mean"]), P(o["rstd"]), m, h, 1e-12, 0.1, 1, 2, None, st)
    fwd_slabs = lambda m, h, ns: L.mtvaf_dropout_res_ln_fwd_slabs(s, ns, s, P(o["x_out"]), s, s, s, P(o["out"]), P(o["mean"]), P(o["rstd"]), m, h,
                                                                  1e-12, 0.1, 1, 2, None, st)
    fwd_planes = lambda m, h, img: L.mtvaf_dropout_res_ln_fwd_planes(s, 0, None, None, s, s, s, P(o["out"]), P(o["mean"]), P(o["rstd"]), m, h,
                                                                     1e-12, 0.1, 1, 2, img, st)
    bwd = lambda m, h, dx, wsb: L.mtvaf_dropout_res_ln_bwd(s, s, s, s, s, s, dx, P(o["dres"]), 0, P(o["dgamma"]), P(o["dbeta"]), P(o["dbias_x"]),
                                                           0, m, h, 0.1, 1, 2, P(o["part"]), wsb, None, st)
    rows = lambda m, h, dx: L.mtvaf_dropout_res_ln_bwd_rows(s, s, s, s, s, s, dx, P(o["dres"]), 0, m, h, 0.1, 1, 2, P(o["part"]), None, st)
    rows_slabs = lambda m, h, ns: L.mtvaf_dropout_res_ln_bwd_rows_slabs(s, s, ns, s, s, s, s, s, P(o["dx"]), P(o["dres"]), 0, m, h, 0.1, 1, 2,
                                                                        P(o["part"]), None, st)
    rows_planes = lambda m, h, img: L.mtvaf_dropout_res_ln_bwd_rows_planes(s, None, 0, s, s, s, s, s, P(o["dx"]), P(o["dres"]), 0, m, h, 0.1, 1,
                                                                           2, P(o["part"]), img, st)
    finish = lambda m, h: L.mtvaf_dropout_res_ln_bwd_finish(P(o["part"]), m, h, P(o["dgamma"]), P(o["dbeta"]), P(o["dbias_x"]), 0, st)
    e_fwd = lambda h: L.mtvaf_embed_ln_fwd(P(ids), P(ids), None, s, s, s, s, s, P(o["out"]), P(o["mean"]), P(o["rstd"]), 1, M, h, 1e-12, 0.1, 1,
                                           2, None, st)
    e_bwd = lambda h, tv, wsb: L.mtvaf_embed_ln_bwd(s, P(ids), P(ids), None, s, s, s, s, s, s, P(o["dword"]), P(o["dpos"]), P(o["dtype"]),
                                                    P(o["dgamma"]), P(o["dbeta"]), 0, 1, M, h, 16, 16, tv, 0, -1, 0.1, 1, 2, P(o["dz"]),
                                                    P(o["ws"]), wsb, st)
    full = 4 * o["part"].numel()
    ews = int(L.mtvaf_embed_ln_bwd_workspace_bytes(M, H, 16, 16))
    assert ews <= 4 * o["ws"].numel()
    cases = [
        ("H=6", ERR_SHAPE, [lambda: fwd(M, 6), lambda: fwd_slabs(M, 6, 1), lambda: bwd(M, 6, P(o["dx"]), full), lambda: rows(M, 6, P(o["dx"])),
                            lambda: rows_slabs(M, 6, 1), lambda: finish(M, 6), lambda: e_fwd(6), lambda: e_bwd(6, 2, ews)]),
        ("H=1028", ERR_SHAPE, [lambda: fwd(M, 1028), lambda: fwd_slabs(M, 1028, 1), lambda: bwd(M, 1028, P(o["dx"]), full),
                               lambda: rows(M, 1028, P(o["dx"])), lambda: rows_slabs(M, 1028, 1), lambda: finish(M, 1028),
                               lambda: e_fwd(1028), lambda: e_bwd(1028, 2, 4 * o["ws"].numel())]),
        ("M=0", ERR_SHAPE, [lambda: fwd(0, H), lambda: fwd_slabs(0, H, 1), lambda: fwd_planes(0, H, P(o["img"])),
                            lambda: bwd(0, H, P(o["dx"]), full), lambda: rows(0, H, P(o["dx"])), lambda: rows_slabs(0, H, 1),
                            lambda: rows_planes(0, H, P(o["img"])), lambda: finish(0, H)]),
        ("nslab=0 for _slabs", ERR_SHAPE, [lambda: fwd_slabs(M, H, 0), lambda: rows_slabs(M, H, 0)]),
        ("H % 32 for _planes", ERR_SHAPE, [lambda: fwd_planes(M, 8, P(o["img"])), lambda: rows_planes(M, 8, P(o["img"]))]),
        ("misaligned plane pointer", ERR_ARG, [lambda: fwd_planes(M, H, P(o["misaligned"])), lambda: rows_planes(M, H, P(o["misaligned"]))]),
        ("dx and dx_bf16 both null", ERR_ARG, [lambda: bwd(M, H, None, full), lambda: rows(M, H, None)]),
        ("type_vocab=3", ERR_SHAPE, [lambda: e_bwd(H, 3, ews)]),
        ("short workspace", ERR_WORKSPACE, [lambda: bwd(M, H, P(o["dx"]), 3 * H * 4 - 1), lambda: e_bwd(H, 2, ews - 1)]),
    ]
    assert o["misaligned"].data_ptr() % 16 == 4
    for name, want, calls in cases:
        for i, fn in enumerate(calls):
            assert fn() == want, (name, i)
    torch.cuda.synchronize()
    assert o.untouched()
