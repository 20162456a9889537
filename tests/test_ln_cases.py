"""The references and bounds of ln_cases.py, proved on the host: ln_ref against F.layer_norm and autograd in float64, the embedding
references against F.embedding with padding_idx, roberta_pos_ref against the oracle, the builders against what their ids promise,
and every bound -- inherited or derived -- against a plain fp32 restatement of the kernels' arithmetic, which must stay within
HEADROOM = 0.25 of it on every case of the tables.

Largest host excess per bound (fp32 restatement / bound, over LN_SHAPES at p = 0.1, the kinds at KIND_SHAPES and EMBED_CASES;
test_fp32_restatement_keeps_four_fold_headroom prints them), measured at this commit:
  y 0.0712   mean 0.1759   rstd 0.1418   dx 0.0159   dres 0.0159   dgamma 0.0405   dbeta 0.0003   dbias_x 0.0026
  embed out 0.0011   dz 0.0010   dword 0.0005   dpos 0.0004   dtype 0.0005   embed dgamma 0.0003   embed dbeta 0.0002
No scale of a case was reduced: tiny stays 1e-20, huge 1e15, the offset 1e3 (the largest the issue keeps as a random case)."""
import numpy as np
import torch
import torch.nn.functional as F

import ln_cases as LC
from oracle import mtvaf_oracle as O

HEADROOM = 0.25


def host_keep(M, H, p, seed):
    """a keep tensor as the device makes them (0 or float32(1 / (1 - p))), from a host generator"""
    if p <= 0:
        return None
    k = (torch.rand(M, H, generator=LC.gen(seed)) >= p).float()
    return k * torch.tensor(LC.dropout_scale(p))


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def test_ln_ref_is_layer_norm_and_its_backward_is_autograd_in_float64():
    for M, H, kind in [(5, 8, "unit"), (3, 260, "offset1e3"), (4, 768, "eps-dominates"), (5, 260, "one-outlier")]:
        x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, kind)
        keep = host_keep(M, H, 0.5, 3)
        xd, rd, gd, bd = (t.double().requires_grad_(True) for t in (x, res, gamma, beta))
        z = xd * keep.double() + rd
        y = F.layer_norm(z, (H,), gd, bd, eps)
        (y * dout.double()).sum().backward()
        ry, mean, rstd, rz = LC.res_ln_ref(x, res, gamma, beta, eps, keep)
        assert torch.allclose(ry, y.detach(), rtol=1e-12, atol=1e-13)
        assert torch.allclose(mean, z.detach().mean(-1), rtol=1e-13, atol=1e-300)
        assert torch.allclose(rstd, (z.detach().var(-1, unbiased=False) + eps).rsqrt(), rtol=1e-12)
        dx, dres, dgamma, dbeta, dbias = LC.res_ln_bwd_ref(dout, x, res, gamma, eps, keep)
        scale = float(rd.grad.abs().max())
        for got, want in ((dx, xd.grad), (dres, rd.grad), (dgamma, gd.grad), (dbeta, bd.grad), (dbias, xd.grad.sum(0))):
            assert float((got - want).abs().max()) <= 1e-9 * max(scale, float(want.abs().max())), (kind, M, H)


def test_embedding_references_are_f_embedding_with_padding_idx():
    for c in (LC.EMBED_CASES[4], LC.EMBED_CASES[13], LC.EMBED_CASES[14], LC.EMBED_CASES[17], LC.EMBED_CASES[18]):
        e = LC.embed_inputs(c)
        H, M = c["H"], e["B"] * e["S"]
        keep = host_keep(M, H, 0.5, 5)
        w, p, t, g, b = (e[k].double().requires_grad_(True) for k in ("word", "pos", "typ", "gamma", "beta"))
        pid = e["pos_ids"].long() if e["pos_ids"] is not None else torch.arange(e["S"])[None, :].expand(e["B"], e["S"])
        z = (F.embedding(e["ids"], w, padding_idx=e["word_pad"]) + F.embedding(e["tts"], t) +
             F.embedding(pid, p, padding_idx=e["pos_pad"] if e["pos_ids"] is not None else None)).reshape(M, H)
        out = F.layer_norm(z, (H,), g, b, e["eps"]) * keep.double()
        (out * e["dout"].double()).sum().backward()
        r_out, mean, rstd, rz = LC.embed_ln_ref(e["ids"], e["tts"], e["pos_ids"], e["word"], e["pos"], e["typ"], e["gamma"], e["beta"],
                                                e["eps"], keep)
        assert torch.equal(rz, z.detach()) and torch.allclose(r_out, out.detach(), rtol=1e-12, atol=1e-13)
        prev = e["prev"] if c["acc"] else None
        got = LC.embed_ln_bwd_ref(e["dout"], e["ids"], e["tts"], e["pos_ids"], e["word"], e["pos"], e["typ"], e["gamma"], e["eps"],
                                  e["word_pad"], e["pos_pad"], keep, prev)[1:]
        for i, (r, want) in enumerate(zip(got, (w.grad, p.grad, t.grad, g.grad, b.grad))):
            want = want + e["prev"][i].double() if c["acc"] else want
            assert torch.allclose(r, want, rtol=1e-10, atol=1e-11), (c["id"], i)
        if c["pad_hits"]:  # the padding rows get nothing
            assert not bool(w.grad[e["word_pad"]].any())
            if e["pos_ids"] is not None:
                assert not bool(p.grad[e["pos_pad"]].any())


def test_roberta_pos_ref_is_the_oracle():
    for S in LC.POS_S:
        ids = LC.pos_ids_inputs(S)
        assert torch.equal(LC.roberta_pos_ref(ids, LC.POS_PAD), O.roberta_position_ids(ids, LC.POS_PAD))
        assert bool((ids[0] != LC.POS_PAD).all()) and bool((ids[1] == LC.POS_PAD).all()) and ids[3, 0] == LC.POS_PAD
        if S > 1:
            assert ids[2, -1] == LC.POS_PAD and ids[2, 0] != LC.POS_PAD
        if S > 65:
            assert all(ids[4, s] == LC.POS_PAD for s in (63, 64)) and ids[4, 66] != LC.POS_PAD
    assert [s for s in LC.POS_S if s > 64 and s % 64] and 64 in LC.POS_S and 128 in LC.POS_S


# ---------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------
def test_shape_table_reaches_every_branch_it_names():
    shapes = {(M, H) for M, H, _ in LC.LN_SHAPES}
    assert all((M, H) in shapes for H in (4, 8, 252, 256, 260, 512, 768, 1020, 1024) for M in (1, 3, 4, 5))
    assert all(H % 4 == 0 and H <= LC.MAX_H for _, H, _ in LC.LN_SHAPES)
    # (csrc/rowops.hip row_grid / row_grid_bwd: the caps these M cross)
    assert 4097 > LC.FWD_GRID_ROWS and 2049 > LC.BWD_GRID_ROWS and 2049 > LC.LEAN_GRID_ROWS
    assert not LC.lean_shape(8) and LC.lean_shape(256) and {(4097, 8), (4097, 256), (2049, 8), (2049, 256)} <= shapes
    assert LC.bwd_blocks(508) == LC.FINISH_WIDE_BLOCKS - 1 and LC.bwd_blocks(509) == LC.FINISH_WIDE_BLOCKS
    assert [LC.lean_shape(H) for H in (256, 512, 768, 1024, 252, 260, 1020)] == [True] * 4 + [False] * 3
    assert any(LC.lean_shape(H) for _, H in LC.KIND_SHAPES) and any(not LC.lean_shape(H) for _, H in LC.KIND_SHAPES)
    assert all(H % 32 == 0 for _, H in LC.PLANE_SHAPES) and [LC.lean_shape(H) for _, H in LC.PLANE_SHAPES] == [False, True]
    assert {H // 64 for _, H in LC.VARIANT_SHAPES if LC.lean_shape(H)} == {4, 8, 12, 16}  # one to four waves


def test_input_kinds_are_what_they_say():
    for M, H in LC.KIND_SHAPES:
        for kind in LC.LN_KINDS:
            x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, kind)
            z = x.double() + res.double()
            y, mean, rstd = LC.ln_ref(z, gamma, beta, eps)
            assert all(bool(torch.isfinite(t.float()).all()) for t in (y, mean, rstd)), kind
            dx, dres, dg, db, dbx = LC.res_ln_bwd_ref(dout, x, res, gamma, eps)
            assert all(bool(torch.isfinite(t.float()).all()) for t in (dx, dg, db, dbx)), kind  # the reference stays in fp32 range
            sd = z.std(-1, unbiased=False)
            if kind == "offset1e3":
                assert bool((mean.abs() > 990).all()) and bool((sd < 2).all()) and float(mean[0]) > 0 > float(mean[1])
            elif kind == "constant-row":
                assert bool((sd == 0).all()) and eps == 1e-5 and torch.equal(y, beta.double().expand(M, H))
                assert torch.allclose(rstd, torch.full((M,), 1e-5 ** -0.5, dtype=torch.float64), rtol=1e-12)
                zf = (x + res)
                assert torch.equal(zf.sum(-1), zf[:, 0] * H)  # exact in fp32 too
            elif kind == "eps-dominates":
                assert bool((sd ** 2 < eps / 100).all()) and eps == 1e-5
            elif kind == "tiny-1e-20":
                assert bool((z.abs().amax(-1) < 1e-19).all()) and float((z.float() ** 2).max()) < 2.0 ** -126
            elif kind == "huge-1e15":
                assert float((z.float() ** 2).sum(-1).max()) < 3e38 and bool((z.abs().amax(-1) > 1e15).all())
            elif kind == "one-outlier":
                assert bool(((z == 1e4).sum(-1) == 1).all())
            elif kind == "gamma0-beta1":
                assert torch.equal(y, torch.ones(M, H, dtype=torch.float64))


def test_embedding_builders_plant_their_segments_zero_rows_and_top_ids():
    ids_seen = [c["id"] for c in LC.EMBED_CASES]
    assert len(set(ids_seen)) == len(ids_seen)
    assert sorted(c["n"] for c in LC.EMBED_CASES[:10]) == [1, 2, 3, 4, 5, 63, 64, 65, 67, 130]
    assert LC.EMBED_TWICE_CASE["n"] == 130 and LC.EMBED_MODE_CASE["n"] == 67
    for c in LC.EMBED_CASES + [LC.EMBED_ATOMIC_CASE]:
        e = LC.embed_inputs(c)
        flat = e["ids"].reshape(-1)
        rows = torch.nonzero(flat == LC.REPEAT).reshape(-1)
        assert len(rows) == c["n"] and torch.equal(rows, e["rep_rows"]), c["id"]
        if c["n"] > 1:
            assert bool((rows[1:] - rows[:-1] > 1).all())  # interleaved: not contiguous in row order
        assert int(flat.max()) < c["vocab"] and int(flat.min()) >= 0
        assert int(e["tts"].max()) < c["type_vocab"] and (c["type_vocab"] == 1 or set(e["tts"].reshape(-1).tolist()) == {0, 1} or c["n"] < 2)
        nz = e["dout"].abs().sum(-1) != 0
        if c["zero"] == "some":
            assert not bool(nz[0]) and not bool(nz[int(rows[-1])]) and not bool(nz[1]) and int(nz[rows].sum()) == c["n"] - 3
            assert bool((e["dout"][~nz].view(torch.int32) == 0).all())  # exact +0
        elif c["zero"] == "all":
            assert not bool(nz.any())
        else:
            assert bool(nz.all())
        if c["top_id"]:
            assert int((flat == c["vocab"] - 1).sum()) == 1
        if c["pad_hits"]:
            assert int((flat == e["word_pad"]).sum()) == 2
        if c["roberta"]:
            assert int(e["pos_ids"].max()) < e["max_pos"] and int((e["pos_ids"] == e["pos_pad"]).sum()) == 2
        else:
            assert e["pos_ids"] is None and e["max_pos"] > e["S"]
    assert LC.EMBED_ATOMIC_CASE["vocab"] > LC.SCAN_MAX_VOCAB
    assert [c["vocab"] for c in LC.EMBED_CASES if c["top_id"]] == [4095, 4096, 4097, LC.SCAN_MAX_VOCAB]


def test_exact_contract_inputs_give_plus_minus_one():
    for M, H in LC.EXACT_SHAPES:
        x, res, gamma, mean, rstd, dout = LC.exact_bwd_inputs(M, H)
        for dtype in (torch.float64, torch.float32):
            dx, dres, _, _, _ = LC.res_ln_bwd_ref(dout, x, res, gamma, 1e-12, None, dtype, stats=(mean, rstd))
            assert torch.equal(dx.abs(), torch.ones(M, H, dtype=dtype)) and torch.equal(dx, dres)
    assert {LC.lean_shape(H) for _, H in LC.EXACT_SHAPES} == {True, False}


def test_keep_scale_forms_agree_except_at_p09():
    """float32(1 / (1 - p)) from the double p -- what mtvaf_dropout, torch and now the LayerNorm kernels multiply by -- against the
    fp32 expression 1.f / (1.f - p) the LayerNorm kernels used: the same bits at 0.1, 0.3 and 0.5 (every result at those p keeps
    its bits), 9.999998 against 10 at 0.9.  The keep threshold is a function of float(p) in both."""
    old = lambda p: np.float32(1) / (np.float32(1) - np.float32(p))
    for p in (0.1, 0.3, 0.5):
        assert old(p).tobytes() == LC.dropout_scale(p).tobytes(), p
    assert LC.dropout_scale(0.9) == np.float32(10.0) and old(0.9) == np.float32(9.999998) != np.float32(10.0)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds: a plain fp32 restatement keeps four-fold headroom on every case
# ---------------------------------------------------------------------------------------------------------------------
def ln_case_excesses(x, res, gamma, beta, dout, eps, keep, cond):
    f32, f64 = torch.float32, torch.float64
    ry, rmean, rstd, z = LC.res_ln_ref(x, res, gamma, beta, eps, keep)
    gy, gmean, grstd, zf = LC.res_ln_ref(x, res, gamma, beta, eps, keep, f32)
    ref = LC.res_ln_bwd_ref(dout, x, res, gamma, eps, keep)
    got = LC.res_ln_bwd_ref(dout, x, res, gamma, eps, keep, f32, stats=(gmean, grstd))  # the kernel reads the fp32 statistics
    t = LC.cond_terms(z, rstd, gamma, dout, keep) if cond else {}
    return {"y": LC.excess(gy, ry, LC.RTOL_ROW, t.get("y")), "mean": LC.mean_excess(gmean, rmean, z),
            "rstd": LC.rstd_excess(grstd, rstd, z), "dx": LC.excess(got[0], ref[0], LC.RTOL_ROW, t.get("dx")),
            "dres": LC.excess(got[1], ref[1], LC.RTOL_ROW, t.get("dx")), "dgamma": LC.excess(got[2], ref[2], LC.RTOL_COL, t.get("dgamma")),
            "dbeta": LC.excess(got[3], ref[3], LC.RTOL_COL), "dbias_x": LC.excess(got[4], ref[4], LC.RTOL_COL, t.get("dbias_x"))}


def test_fp32_restatement_keeps_four_fold_headroom():
    worst = {}

    def note(tag, ex):
        for k, v in ex.items():
            assert v <= HEADROOM, (tag, k, v)
            worst[k] = max(worst.get(k, 0.0), v)

    for M, H, why in LC.LN_SHAPES:
        x, res, gamma, beta, dout, eps = LC.ln_inputs(M, H, "unit")
        note((M, H), ln_case_excesses(x, res, gamma, beta, dout, eps, host_keep(M, H, LC.LN_P, M + H), False))
    for M, H in LC.KIND_SHAPES:
        for kind in LC.LN_KINDS:
            note((M, H, kind), ln_case_excesses(*LC.ln_inputs(M, H, kind), None, kind in LC.COND_KINDS))
    for c in LC.EMBED_CASES + [LC.EMBED_ATOMIC_CASE]:
        e = LC.embed_inputs(c)
        keep = host_keep(e["B"] * e["S"], c["H"], c["p"], 7)
        a = (e["ids"], e["tts"], e["pos_ids"], e["word"], e["pos"], e["typ"], e["gamma"])
        prev = e["prev"] if c["acc"] else None
        r_out, r_mean, r_rstd, z = LC.embed_ln_ref(*a, e["beta"], e["eps"], keep)
        g_out, g_mean, g_rstd, _ = LC.embed_ln_ref(*a, e["beta"], e["eps"], keep, torch.float32)
        ref = LC.embed_ln_bwd_ref(e["dout"], *a, e["eps"], e["word_pad"], e["pos_pad"], keep, prev)
        got = LC.embed_ln_bwd_ref(e["dout"], *a, e["eps"], e["word_pad"], e["pos_pad"], keep, prev, torch.float32)
        ex = {"embed out": LC.excess(g_out, r_out, LC.RTOL_ROW), "mean": LC.mean_excess(g_mean, r_mean, z),
              "rstd": LC.rstd_excess(g_rstd, r_rstd, z), "dz": LC.excess(got[0], ref[0], LC.RTOL_ROW)}
        for i, name in enumerate(("dword", "dpos", "dtype", "embed dgamma", "embed dbeta")):
            ex[name] = LC.excess(got[1 + i], ref[1 + i], LC.RTOL_COL)
        note(c["id"], ex)
    print("fp32 restatement, largest excess per bound:", {k: round(v, 4) for k, v in worst.items()})
    # a wrong statistic does not pass: the mean off by 1e-3 of sigma and rstd off by 1e-3 of itself at the offset case (1e-5 at unit scale)
    x, res, gamma, beta, dout, eps = LC.ln_inputs(5, 260, "offset1e3")
    ry, rmean, rstd, z = LC.res_ln_ref(x, res, gamma, beta, eps)
    assert LC.mean_excess((rmean + 1e-3).float(), rmean, z) > 1 and LC.rstd_excess((rstd * (1 + 1e-3)).float(), rstd, z) > 1
    xu, ru, gu, bu, _, eu = LC.ln_inputs(5, 260, "unit")
    _, _, rstd_u, zu = LC.res_ln_ref(xu, ru, gu, bu, eu)
    assert LC.rstd_excess((rstd_u * (1 + 1e-5)).float(), rstd_u, zu) > 1
    t = LC.cond_terms(z, rstd, gamma, dout)
    assert LC.excess((ry + 2e-3).float(), ry, LC.RTOL_ROW, t["y"]) > 1
    # and a tensor of the order of 1e-15 is not compared against the constant 1e-7 of `close`
    small = torch.full((4,), 1e-15, dtype=torch.float64)
    assert LC.excess((small * 1.01).float(), small, LC.RTOL_ROW) > 1 >= LC.excess(small.float(), small, LC.RTOL_ROW)
