"""The streaming, packing and prompt kernels against the float64 references of stream_cases.py (whose case tables and bounds
test_stream_cases.py proves on the host): the optimizer, the bf16 gradient wire format, the prompt-generator pieces, the packing
helpers, the column sums, the bf16 cast and dropout, each at the sizes where its vector width, its capped grid or its dispatch
takes another path.  Rejections are tested only where the entry point returns before it launches anything."""
import numpy as np
import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_ = SC.SENTINEL


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def call(hip, name, *args):
    hip._ck(getattr(hip.lib(), name)(*args, hip._st()), name)


def views_on_device(sizes_shifts, dtype=torch.float32):
    """one allocation filled with the sentinel -> (buffer, views, guard mask)"""
    offs, total = SC.view_layout(sizes_shifts, align=16 // torch.empty(0, dtype=dtype).element_size())
    buf = torch.full((total,), S_, dtype=dtype, device=DEV)
    sizes = [n for n, _ in sizes_shifts]
    return buf, [buf[o:o + n] for o, n in zip(offs, sizes)], SC.guard_mask(total, offs, sizes)


def guards_intact(buf, guard):
    return bool((buf.cpu().float()[guard] == S_).all())


def check_adam_step(got, old, g, lr, wd, step, gscale, tag):
    ref = SC.adamw_ref(old[0], g, old[1], old[2], lr, wd, step, gscale)
    err = SC.adam_errors(got, ref, old[0], old[1], g, lr, gscale)
    print(tag, {k: round(e, 4) for k, e in err.items()})
    for k, e in err.items():
        assert e <= SC.ADAM_DEVICE_FACTOR * SC.ADAM_F32_ERR[k], (tag, k, e)


# ---------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.ADAM_CASES, ids=[c[0] for c in SC.ADAM_CASES])
def test_adamw(hip, case):
    cid, n, shifts, shadow, max_blocks, hyper, gscale = case
    lr, wd, step0, zero = SC.ADAM_HYPER[hyper]
    p, m, v, gs = SC.adam_inputs(n, zero, seed=n)
    buf, (vp, vg, vm, vv), guard = views_on_device([(n, s) for s in shifts])
    assert [t.data_ptr() % 16 for t in (vp, vg, vm, vv)] == [4 * s for s in shifts]
    vp.copy_(p), vm.copy_(m), vv.copy_(v)
    sbuf = sv = None
    if shadow is not None:
        sbuf, (sv,), sguard = views_on_device([(n, shadow)], dtype=torch.bfloat16)
        assert sv.data_ptr() % 16 == 2 * shadow
    old = (p, m, v)
    for k, g in enumerate(gs):  # two consecutive steps
        vg.copy_(g)
        hip.adamw(vp, vg, vm, vv, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step0 + k, grad_scale=gscale, p_bf16=sv, max_blocks=max_blocks)
        got = (vp.cpu(), vm.cpu(), vv.cpu())
        check_adam_step(got, old, g, lr, wd, step0 + k, gscale, "%s step %d" % (cid, step0 + k))
        assert torch.equal(vg.cpu(), g)
        if sv is not None:  # the shadow is the new parameter rounded to bf16, bit for bit
            assert torch.equal(SC.bits16(sv.cpu()), SC.bits16(got[0].to(torch.bfloat16)))
            assert guards_intact(sbuf, sguard)
        assert guards_intact(buf, guard)
        old = got


@pytest.mark.parametrize("case", SC.ADAM_MULTI_CASES, ids=[c[0] for c in SC.ADAM_MULTI_CASES])
def test_adamw_multi(hip, case):
    cid, count, big = case
    lr, wd, step = SC.ADAM_MULTI_HYPER
    members = SC.adam_multi_members(count, big)
    layout = [(n, s) for n, s in members for _ in range(4)]
    offs, total = SC.view_layout(layout)
    host = torch.full((total,), S_)
    ins = []
    for i, (n, s) in enumerate(members):
        p, m, v, (g, _) = SC.adam_inputs(n, False, seed=1000 * count + i)
        ins.append((p, g, m, v))
        for j, t in enumerate((p, g, m, v)):
            host[offs[4 * i + j]:offs[4 * i + j] + n] = t
    buf = host.to(DEV)
    view = lambda i, j: buf[offs[4 * i + j]:offs[4 * i + j] + members[i][0]]
    ps, gs, ms, vs = ([view(i, j) for i in range(count)] for j in range(4))
    assert all(t.data_ptr() % 16 == 4 * s for t, (_, s) in zip(ps, members))
    hip.adamw_multi(ps, gs, ms, vs, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step)
    out = buf.cpu()
    worst = {k: 0.0 for k in SC.ADAM_F32_ERR}
    for i, (n, s) in enumerate(members):
        p, g, m, v = ins[i]
        got = tuple(out[offs[4 * i + j]:offs[4 * i + j] + n] for j in (0, 2, 3))
        assert torch.equal(out[offs[4 * i + 1]:offs[4 * i + 1] + n], g)
        err = SC.adam_errors(got, SC.adamw_ref(p, g, m, v, lr, wd, step), p, m, g, lr)
        for k, e in err.items():
            worst[k] = max(worst[k], e)
            assert e <= SC.ADAM_DEVICE_FACTOR * SC.ADAM_F32_ERR[k], (cid, i, n, s, k, e)
    print(cid, {k: round(e, 4) for k, e in worst.items()})
    assert bool((out[SC.guard_mask(total, offs, [n for n, _ in layout])] == S_).all())


def test_adamw_multi_count0_returns_without_a_launch(hip):
    assert hip.lib().mtvaf_adamw_multi(0, None, None, None, None, None, 1e-3, SC.BETA1, SC.BETA2, SC.EPS, 1e-2, 0.1, 0.1, 1.0,
                                       hip._st()) == 0
    hip.adamw_multi([], [], [], [], 1e-3, SC.BETA1, SC.BETA2, SC.EPS, 1e-2, 1)


def test_adamw_planes_update_and_rejections(hip):
    lr, wd, step = SC.PLANES_HYPER
    n = sum(r * c for r, c in SC.PLANES_SHAPES) + sum(SC.PLANES_GAPS)
    p, m, v, (g, _) = SC.adam_inputs(n, False, seed=3)
    segs, off = [], 0
    for (r, c), gap in zip(SC.PLANES_SHAPES, SC.PLANES_GAPS):
        segs.append((off, r, c, torch.full((6 * r * c,), 0x7f, dtype=torch.uint8, device=DEV)))
        off += r * c + gap
    dp, dg, dm, dv = (t.to(DEV) for t in (p, g, m, v))
    hip.adamw_planes(dp, dg, dm, dv, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step, segs, max_blocks=3)
    check_adam_step((dp.cpu(), dm.cpu(), dv.cpu()), (p, m, v), g, lr, wd, step, 1.0, "planes max_blocks 3")
    small = [torch.ones(6, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError):  # n % 4 != 0
        hip.adamw_planes(*small, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step, [])
    flat = [torch.ones(192, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError):  # cols % 32 != 0
        hip.adamw_planes(*flat, lr, SC.BETA1, SC.BETA2, SC.EPS, wd, step,
                         [(0, 4, 48, torch.zeros(6 * 192, dtype=torch.uint8, device=DEV))])
    assert all(bool((t == 1).all()) for t in small + flat)


# ---------------------------------------------------------------------------------------------------------------------
# bf16 wire format
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,extra", SC.PACK_CASES, ids=["n%d-pad%d" % c for c in SC.PACK_CASES])
def test_grad_pack_bf16(hip, n, extra):
    npad = (n + 7) // 8 * 8 + extra
    x = SC.planted_f32(n, seed=n)
    dst = torch.full((npad + 16,), S_, dtype=torch.bfloat16, device=DEV)
    hip.grad_pack_bf16(x.to(DEV), dst, n, npad)
    out = dst.cpu()
    assert SC.same_bf16(out[:n], SC.bf16_round_ref(x))
    assert bool((SC.bits16(out[n:npad]) == 0).all())  # +0 fills [n, npad)
    assert bool((out[npad:].float() == S_).all())


def test_grad_pack_bf16_rejections(hip):
    x, dst = torch.ones(16, device=DEV), torch.full((32,), S_, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        hip.grad_pack_bf16(x, dst, 9, 12)  # npad % 8 != 0
    with pytest.raises(RuntimeError):
        hip.grad_pack_bf16(x, dst, 9, 8)   # npad < n
    assert bool((dst.float() == S_).all())


@pytest.mark.parametrize("W,chunk,scale", SC.REDUCE_CASES, ids=["W%d-chunk%d-scale%g" % c for c in SC.REDUCE_CASES])
def test_grad_reduce_bf16(hip, W, chunk, scale):
    recv = SC.reduce_inputs(W, chunk, seed=W)
    out = torch.full((chunk + 16,), S_, dtype=torch.bfloat16, device=DEV)
    hip.grad_reduce_bf16(recv.to(DEV), out, W, chunk, scale)
    got = out.cpu()
    assert SC.same_bf16(got[:chunk], SC.reduce_ref(recv, W, chunk, scale))
    assert bool((got[chunk:].float() == S_).all())


@pytest.mark.parametrize("n", SC.UNPACK_CASES)
def test_grad_unpack_bf16(hip, n):
    src = SC.unpack_inputs(n, seed=n)
    dst = torch.full((n + 16,), S_, device=DEV)
    hip.grad_unpack_bf16(src.to(DEV), dst, n)
    got = dst.cpu()
    assert torch.equal(got[:n].view(torch.int32), src[:n].float().view(torch.int32))
    assert bool((got[n:] == S_).all())  # elements past n are untouched


# ---------------------------------------------------------------------------------------------------------------------
# prompt pieces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,W", SC.SPLIT_MEAN_CASES, ids=[SC.split_mean_id(c) for c in SC.SPLIT_MEAN_CASES])
def test_split_mean(hip, rows, W):
    enc = torch.randn(rows * 4 * W, generator=SC.gen(rows))
    sm = torch.full((rows * W + 8,), S_, device=DEV)
    genc = enc.to(DEV)
    call(hip, "mtvaf_split_mean", hip._p(genc), hip._p(sm), rows, W)
    assert SC.close_excess(sm[:rows * W].view(rows, W), SC.split_mean_ref(enc, rows, W), SC.RTOL_SPLIT_MEAN) <= 1
    assert bool((sm[rows * W:] == S_).all())


def test_split_mean_rejects_w_not_a_multiple_of_4(hip):
    enc, sm = torch.ones(4 * 6, device=DEV), torch.full((8,), S_, device=DEV)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_split_mean", hip._p(enc), hip._p(sm), 1, 6)
    assert bool((sm == S_).all())


@pytest.mark.parametrize("mode", SC.GATE_MODES)
@pytest.mark.parametrize("ngroups", SC.GATE_GROUPS)
def test_gate_fwd(hip, ngroups, mode):
    z = SC.gate_logits(ngroups, mode)
    gate = torch.full((ngroups * 4 + 8,), S_, device=DEV)
    gz = z.to(DEV)
    call(hip, "mtvaf_gate_fwd", hip._p(gz), hip._p(gate), ngroups)
    got = gate[:ngroups * 4].view(ngroups, 4).cpu()
    excess = SC.norm_excess(got, SC.gate_ref(z), SC.RTOL_GATE)
    print("gate", ngroups, mode, "excess", round(excess, 4))
    assert excess <= 1
    assert float((got.double().sum(-1) - 1).abs().max()) <= SC.GATE_SUM_TOL  # every group sums to 1 within fp32
    if mode in ("all-equal", "minus1e4-constant"):
        assert bool((got == 0.25).all())
    assert bool((gate[ngroups * 4:] == S_).all())


@pytest.mark.parametrize("case", SC.MIX_CASES, ids=[SC.mix_id(c) for c in SC.MIX_CASES])
def test_prompt_mix_chain(hip, case):
    NL, NI, B, Lp, W = case
    n, hid = NI * B, W // 2
    enc, z, gk, dsm = SC.mix_inputs(*case)
    r_sm, r_gate, r_pkv, r_dz, r_denc = SC.mix_ref(enc, z, gk, dsm, *case)
    genc, gz, ggk, gdsm = (t.to(DEV) for t in (enc, z, gk, dsm))
    p = hip._p
    sm = torch.empty(n, Lp * W, device=DEV)
    call(hip, "mtvaf_split_mean", p(genc), p(sm), n * Lp, W)
    assert SC.close_excess(sm, r_sm, SC.RTOL_SPLIT_MEAN) <= 1
    gate = torch.empty(n, NL * 4, device=DEV)
    call(hip, "mtvaf_gate_fwd", p(gz), p(gate), n * NL)
    assert SC.norm_excess(gate, r_gate, SC.RTOL_GATE) <= 1
    pkv = torch.full((NL * 2 * B * NI * Lp * hid + 8,), S_, device=DEV)
    call(hip, "mtvaf_prompt_mix_fwd", p(genc), p(gate), p(pkv), NI, B, Lp, W, NL)
    assert SC.close_excess(pkv[:-8].view(NL, 2, B, -1), r_pkv, SC.RTOL_MIX_FWD) <= 1
    assert bool((pkv[-8:] == S_).all())
    dpart = torch.empty(n * Lp, NL * 4, device=DEV)
    dlog = torch.full((n * NL * 4 + 8,), S_, device=DEV)
    call(hip, "mtvaf_prompt_mix_bwd_gate", p(genc), p(ggk), p(gz), p(gate), p(dpart), p(dlog), NI, B, Lp, W, NL)
    assert SC.close_excess(dlog[:-8].view(n, NL * 4), r_dz, SC.RTOL_MIX_GRAD) <= 1
    assert bool((dlog[-8:] == S_).all())
    denc = torch.full((NI * B * Lp * 4 * W + 8,), S_, device=DEV)
    call(hip, "mtvaf_prompt_mix_bwd_enc", p(gate), p(ggk), p(gdsm), p(denc), NI, B, Lp, W, NL)
    assert SC.close_excess(denc[:-8].view(NI, B, Lp, 4 * W), r_denc, SC.RTOL_MIX_GRAD) <= 1
    assert bool((denc[-8:] == S_).all())


@pytest.mark.parametrize("NL,W", SC.MIX_REJECTED, ids=["NL%d-W%d" % c for c in SC.MIX_REJECTED])
def test_prompt_mix_rejects_depths_and_widths_it_has_no_kernel_for(hip, NL, W):
    NI, B, Lp = 2, 2, 2
    n = NI * B
    big = lambda *s: torch.full(s, S_, device=DEV)
    enc, gate, z = big(NI, B, Lp, 4 * W), big(n, NL * 4), big(n, NL * 4)
    pkv, dsm = big(NL, 2, B, NI * Lp * (W // 2 + 1)), big(n, Lp * W)
    dpart, dlog, denc = big(n * Lp, NL * 4), big(n, NL * 4), big(NI, B, Lp, 4 * W)
    p = hip._p
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_prompt_mix_fwd", p(enc), p(gate), p(pkv), NI, B, Lp, W, NL)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_prompt_mix_bwd_gate", p(enc), p(pkv), p(z), p(gate), p(dpart), p(dlog), NI, B, Lp, W, NL)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_prompt_mix_bwd_enc", p(gate), p(pkv), p(dsm), p(denc), NI, B, Lp, W, NL)
    assert all(bool((t == S_).all()) for t in (pkv, dpart, dlog, denc))


@pytest.mark.parametrize("mode", SC.KL_LOGITS)
@pytest.mark.parametrize("B,N", SC.KL_SHAPES, ids=["B%d-N%d" % s for s in SC.KL_SHAPES])
def test_kl_logsoftmax_cases(hip, B, N, mode):
    z, t = SC.kl_inputs(B, N, mode)
    r_loss, r_dz = SC.kl_ref(z, t)
    gz, gt = z.to(DEV), t.to(DEV)
    p = hip._p
    loss, row = torch.full((1,), S_, device=DEV), torch.full((B + 8,), S_, device=DEV)
    call(hip, "mtvaf_kl_logsoftmax_fwd", p(gz), p(gt), p(loss), p(row), B, N)
    dz = torch.full((B * N + 8,), S_, device=DEV)
    gout = torch.tensor([SC.KL_GOUT], device=DEV)
    call(hip, "mtvaf_kl_logsoftmax_bwd", p(gout), SC.KL_GSCALE, p(gz), p(gt), p(dz), B, N)
    e_loss = SC.close_excess(loss, r_loss.reshape(1), SC.RTOL_KL_LOSS)
    e_dz = SC.close_excess(dz[:-8].view(B, N), r_dz, SC.RTOL_KL_GRAD, SC.ATOL_KL_GRAD)
    print(SC.kl_id(B, N, mode), "loss excess", round(e_loss, 4), "gradient excess", round(e_dz, 4))
    assert e_loss <= 1 and e_dz <= 1
    rows, grad = row.cpu(), dz[:-8].view(B, N).cpu()
    for r in range(B):
        if SC.KL_TARGET_KINDS[(r + N) % 5] == "all-zero":  # exactly nothing from an all-zero target row
            assert float(rows[r]) == 0.0 and not bool(grad[r].any())
    assert bool((rows[B:] == S_).all()) and bool((dz[-8:] == S_).all())


@pytest.mark.parametrize("case", SC.MEAN_L_CASES, ids=[SC.mean_l_id(c) for c in SC.MEAN_L_CASES])
def test_mean_l_fwd_and_accumulating_bwd(hip, case):
    n, L, W4 = case
    enc, dmean, prior = SC.mean_l_inputs(n, L, W4)
    genc, gdm = enc.to(DEV), dmean.to(DEV)
    p = hip._p
    out = torch.full((n * W4 + 8,), S_, device=DEV)
    call(hip, "mtvaf_mean_l_fwd", p(genc), p(out), n, L, W4)
    assert SC.norm_excess(out[:-8].view(n, W4), enc.double().mean(1), SC.RTOL_MEAN_L) <= 1
    denc = torch.full((n * L * W4 + 8,), S_, device=DEV)
    denc[:-8].copy_(prior.reshape(-1))
    call(hip, "mtvaf_mean_l_bwd", p(gdm), p(denc), n, L, W4)  # accumulates: prior + dmean / L
    want = prior.double() + dmean.double()[:, None, :] / L
    assert SC.norm_excess(denc[:-8].view(n, L, W4), want, SC.RTOL_MEAN_L) <= 1
    assert bool((out[-8:] == S_).all()) and bool((denc[-8:] == S_).all())


def test_mean_l_rejects_w4_not_a_multiple_of_4(hip):
    a, b = torch.ones(2 * 6, device=DEV), torch.full((8,), S_, device=DEV)
    p = hip._p
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_mean_l_fwd", p(a), p(b), 1, 2, 6)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_mean_l_bwd", p(b), p(a), 1, 2, 6)
    assert bool((b == S_).all()) and bool((a == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def run_packing(hip, m, B, S, P, ordered, T=None):
    gm = m.to(DEV)
    i32 = lambda k: torch.full((k + 4,), -7, dtype=torch.int32, device=DEV)
    cu, inv, rowmap, mv = i32(2 * B + 1), i32(B * S), i32(B * S), i32(1)
    p = hip._p
    call(hip, "mtvaf_build_packing_ordered" if ordered else "mtvaf_build_packing", p(gm), B, P + S if T is None else T, P, S, p(cu),
         p(inv), p(rowmap), p(mv))
    return cu, inv, rowmap, mv


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "ordered"])
@pytest.mark.parametrize("case", SC.PACK_MASK_CASES, ids=[c[0] for c in SC.PACK_MASK_CASES])
def test_build_packing(hip, case, ordered):
    _, B, S, P, kind, masked, pm = case
    m = SC.packing_mask(B, S, P, kind, masked, pm)
    r_cu, r_inv, r_rowmap, r_mv = SC.packing_ref(m, P, S, ordered)
    cu, inv, rowmap, mv = (t.cpu().numpy() for t in run_packing(hip, m, B, S, P, ordered))
    assert np.array_equal(cu[:len(r_cu)], r_cu) and (cu[len(r_cu):] == -7).all()
    assert np.array_equal(inv[:B * S], r_inv) and (inv[B * S:] == -7).all()
    assert np.array_equal(rowmap[:B * S], r_rowmap) and (rowmap[B * S:] == -7).all()
    assert mv[0] == r_mv and (mv[1:] == -7).all()


def test_build_packing_rejects_t_other_than_p_plus_s(hip):
    m = SC.packing_mask(2, 64, 4, "holes", -10000.0, False)
    for ordered in (False, True):
        with pytest.raises(RuntimeError):
            run_packing(hip, m, 2, 64, 4, ordered, T=4 + 64 - 1)


@pytest.mark.parametrize("pattern", SC.KTILE_PATTERNS)
@pytest.mark.parametrize("bk,B,S", SC.KTILE_SHAPES, ids=["bk%d-B%d-S%d" % s for s in SC.KTILE_SHAPES])
def test_build_ktiles(hip, bk, B, S, pattern):
    m = SC.ktile_mask(bk, B, S, pattern)
    live, cnt = SC.ktiles_ref(m, SC.KTILE_P, S, bk)
    nt = B * S // bk
    gm = m.to(DEV)
    klist = torch.full((nt + 4,), -7, dtype=torch.int32, device=DEV)
    kcnt = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    call(hip, "mtvaf_build_ktiles", hip._p(gm), B, SC.KTILE_P + S, SC.KTILE_P, S, bk, hip._p(klist), hip._p(kcnt))
    kl, kc = klist.cpu().numpy(), kcnt.cpu().numpy()
    assert kc[0] == cnt and (kc[1:] == -7).all(), SC.ktile_id(bk, B, S, pattern)
    assert np.array_equal(kl[:cnt], live) and (kl[cnt:] == -7).all(), SC.ktile_id(bk, B, S, pattern)
    if pattern == "all-live":  # the wrapper, as the engine calls it
        wl, wc = hip.build_ktiles(gm, SC.KTILE_P, S, bk)
        assert int(wc) == cnt and np.array_equal(wl.cpu().numpy()[:cnt], live)


def test_build_ktiles_rejects_a_token_axis_that_is_no_multiple_of_bk(hip):
    m = SC.ktile_mask(32, 1, 32, "all-live").to(DEV)
    klist, kcnt = torch.full((4,), -7, dtype=torch.int32, device=DEV), torch.full((4,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_build_ktiles", hip._p(m), 1, SC.KTILE_P + 32, SC.KTILE_P, 32, 64, hip._p(klist), hip._p(kcnt))
    assert bool((klist == -7).all()) and bool((kcnt == -7).all())


def gather(hip, src, mp, rows, H):
    dst = torch.full((rows * H + 8,), S_, device=DEV)
    call(hip, "mtvaf_gather_rows", hip._p(src), hip._p(mp), hip._p(dst), rows, H)
    assert bool((dst[-8:] == S_).all())
    return dst[:-8].view(rows, H)


@pytest.mark.parametrize("kind", SC.GATHER_MAPS)
@pytest.mark.parametrize("rows,H", SC.GATHER_CASES, ids=["rows%d-H%d" % c for c in SC.GATHER_CASES])
def test_gather_rows(hip, rows, H, kind):
    src, mp = SC.gather_inputs(rows, H, kind)
    got = gather(hip, src.to(DEV), mp.to(DEV), rows, H).cpu()
    assert torch.equal(got.view(torch.int32), SC.gather_ref(src, mp).view(torch.int32))


def test_gather_rows_packs_and_unpacks_through_the_maps_of_a_packing_case(hip):
    _, B, S, P, kind, masked, pm = SC.PACK_MASK_CASES[5]
    m = SC.packing_mask(B, S, P, kind, masked, pm)
    cu, inv, rowmap, mv = run_packing(hip, m, B, S, P, False)
    H = 8
    x = torch.randn(B * S, H, generator=SC.gen(9))
    gx = x.to(DEV)
    packed = gather(hip, gx, rowmap, B * S, H)
    back = gather(hip, packed, inv, B * S, H).cpu()
    keep = (m[:, P:] > -5000).reshape(-1)
    assert int(mv[0]) == int(keep.sum()) and bool((packed[int(mv[0]):] == 0).all())
    assert torch.equal(back[keep], x[keep]) and not bool(back[~keep].any())


def test_gather_rows_rejects_h_not_a_multiple_of_4(hip):
    src, mp, dst = torch.ones(2, 6, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.full((16,), S_, device=DEV)
    with pytest.raises(RuntimeError):
        call(hip, "mtvaf_gather_rows", hip._p(src), hip._p(mp), hip._p(dst), 2, 6)
    assert bool((dst == S_).all())


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-one-float-scalar-path"])
@pytest.mark.parametrize("n", SC.ZERO_SIZES)
def test_zero_f32(hip, n, shift):
    buf, (v,), guard = views_on_device([(n, shift)])
    assert v.data_ptr() % 16 == 4 * shift
    call(hip, "mtvaf_zero_f32", hip._p(v), n)
    assert bool((v.view(torch.int32) == 0).all())
    assert guards_intact(buf, guard)


def test_zero_f32_of_nothing_is_a_no_op(hip):
    buf = torch.full((16,), S_, device=DEV)
    call(hip, "mtvaf_zero_f32", hip._p(buf), 0)
    call(hip, "mtvaf_zero_f32", None, 0)
    assert bool((buf == S_).all())


# ---------------------------------------------------------------------------------------------------------------------
# reductions, casts, dropout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", SC.COLSUM_ROWS, ids=[SC.colsum_id(r) for r in SC.COLSUM_ROWS])
def test_colsum_on_both_sides_of_the_kernel_switch(hip, rows):
    for cols in SC.COLSUM_COLS:
        x, prior = SC.colsum_inputs(rows, cols)
        gx = x.to(DEV)
        for acc in (False, True):
            out = torch.full((cols + 8,), S_, device=DEV)
            out[:cols].copy_(prior)
            hip.colsum(gx, out[:cols], accumulate=acc)
            ref = x.double().sum(0) + (prior.double() if acc else 0)
            assert SC.close_excess(out[:cols], ref, SC.RTOL_COLSUM) <= 1, (rows, cols, acc)
            assert bool((out[cols:] == S_).all())


@pytest.mark.parametrize("rows,cols,ld", SC.COLSUM_STRIDED, ids=["rows%d-cols%d-ld%d" % c for c in SC.COLSUM_STRIDED])
def test_colsum_with_a_leading_dimension_larger_than_the_width(hip, rows, cols, ld):
    x, prior = SC.colsum_inputs(rows, cols, ld)
    gx = x.to(DEV)
    for acc in (False, True):
        out = prior.to(DEV)
        hip.colsum(gx[:, :cols], out, accumulate=acc)
        ref = x[:, :cols].double().sum(0) + (prior.double() if acc else 0)
        assert SC.close_excess(out, ref, SC.RTOL_COLSUM) <= 1, acc


@pytest.mark.parametrize("rows", SC.COLSUM_SMALL_ROWS)
def test_colsum_small(hip, rows):
    for cols in SC.COLSUM_SMALL_COLS:
        x, prior = SC.colsum_inputs(rows, cols)
        gx = x.to(DEV)
        for acc in (False, True):
            out = torch.full((cols + 8,), S_, device=DEV)
            out[:cols].copy_(prior)
            hip.colsum_small(gx, out[:cols], accumulate=acc)
            ref = x.double().sum(0) + (prior.double() if acc else 0)
            assert SC.close_excess(out[:cols], ref, SC.RTOL_COLSUM) <= 1, (rows, cols, acc)
            assert bool((out[cols:] == S_).all())


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "all-three-leading-dimensions-padded"])
@pytest.mark.parametrize("outputs", SC.CAST_OUTPUTS)
@pytest.mark.parametrize("R,C", SC.CAST_SHAPES, ids=["R%d-C%d" % s for s in SC.CAST_SHAPES])
def test_cast_bf16(hip, R, C, outputs, strided):
    x = SC.cast_inputs(R, C)
    px, po, pt = SC.CAST_PADS if strided else (0, 0, 0)
    gx = torch.full((R, C + px), S_, device=DEV)
    gx[:, :C].copy_(x)
    out = torch.full((R, C + po), S_, dtype=torch.bfloat16, device=DEV)
    out_t = torch.full((C, R + pt), S_, dtype=torch.bfloat16, device=DEV)
    hip.cast_bf16(gx[:, :C], out=out[:, :C] if outputs != "out_t" else None, out_t=out_t[:, :R] if outputs != "out" else None)
    want = SC.bf16_round_ref(x.reshape(-1)).view(R, C)
    o, ot = out.cpu(), out_t.cpu()
    if outputs != "out_t":
        assert SC.same_bf16(o[:, :C], want)
    else:
        assert bool((o.float() == S_).all())
    if outputs != "out":
        assert SC.same_bf16(ot[:, :R], want.t())
    else:
        assert bool((ot.float() == S_).all())
    # the bytes between the rows of a strided output are untouched
    assert bool((o[:, C:].float() == S_).all()) and bool((ot[:, R:].float() == S_).all())


def run_dropout(hip, x, p, seed, offset):
    out = torch.full((x.numel() + 8,), S_, device=DEV)
    hip.dropout(x, out[:-8], p, seed, offset)
    assert bool((out[-8:] == S_).all())
    return out[:-8].cpu()


@pytest.mark.parametrize("p", SC.DROPOUT_PS)
def test_dropout_keep_fraction_lanes_and_scale(hip, p):
    n = SC.DROPOUT_N
    x = torch.randn(n, generator=SC.gen(1)).abs() + 0.5
    y = run_dropout(hip, x.to(DEV), p, 1234, 5)
    keep = y != 0
    frac = float(keep.double().mean())
    lanes = [float(keep[i::4].double().mean()) for i in range(4)]
    print("dropout p", p, "kept", frac, "lanes", lanes)
    assert abs(frac - (1 - p)) <= SC.keep_fraction_bound(p, n)
    for i in range(4):  # each of the four lane bits of dropout_keep4 is fair
        assert abs(lanes[i] - (1 - p)) <= SC.keep_fraction_bound(p, n // 4), i
    scaled = x * torch.tensor(SC.dropout_scale(p))
    assert torch.equal(y[keep].view(torch.int32), scaled[keep].view(torch.int32))  # bit for bit


def test_dropout_mask_depends_on_seed_offset_and_index_only(hip):
    ones = torch.ones(8192, device=DEV)
    a = run_dropout(hip, ones[:4096], 0.5, 77, 3) != 0
    b = run_dropout(hip, ones, 0.5, 77, 3) != 0
    assert torch.equal(a, b[:4096])  # the mask of element i does not depend on n
    assert not torch.equal(b, run_dropout(hip, ones, 0.5, 78, 3) != 0)
    assert not torch.equal(b, run_dropout(hip, ones, 0.5, 77, 4) != 0)
    assert torch.equal(b, run_dropout(hip, ones, 0.5, 77, 3) != 0)


def test_dropout_stride_loop_writes_every_element(hip):
    n, p = SC.DROPOUT_STRIDE_N, 0.5
    y = run_dropout(hip, torch.ones(n, device=DEV), p, 9, 0)
    scale = float(SC.dropout_scale(p))
    assert bool(((y == 0) | (y == scale)).all())
    assert abs(float((y != 0).double().mean()) - (1 - p)) <= SC.keep_fraction_bound(p, n)


def test_dropout_p0_copies_and_n_must_be_a_multiple_of_4(hip):
    x = torch.randn(4100, generator=SC.gen(2))
    assert torch.equal(run_dropout(hip, x.to(DEV), 0.0, 1, 1), x)
    gx = x.to(DEV)
    hip.dropout(gx, gx, 0.0, 1, 1)  # in place
    assert torch.equal(gx.cpu(), x)
    out = torch.full((8,), S_, device=DEV)
    with pytest.raises(RuntimeError):
        hip.dropout(gx[:6], out, 0.5, 1, 1)
    assert bool((out == S_).all())
