"""The references and tolerances of stream_cases.py, proved on the host against independent statements (torch.optim.AdamW,
nonzero + stable sort, Python loops, Tensor.to(bfloat16), F.kl_div, the einsum of test_prompt_mix), and the headroom of every
inherited bound: a plain fp32 restatement of each formula meets it four times over on every case of the tables."""
import numpy as np
import torch
import torch.nn.functional as F

import stream_cases as SC

HEADROOM = 0.25


def adam_case_steps():
    """every (p_old, g, m, v, lr, wd, step, grad_scale) the GPU tests feed a kernel, the second step taken from the fp32
    restatement's state"""
    runs = []
    for cid, n, _, _, _, hyper, gs in SC.ADAM_CASES:
        lr, wd, step, zero = SC.ADAM_HYPER[hyper]
        runs.append((cid, SC.adam_inputs(n, zero, seed=n), lr, wd, step, gs))
    for cid, count, big in SC.ADAM_MULTI_CASES:
        lr, wd, step = SC.ADAM_MULTI_HYPER
        for i, (n, _) in enumerate(SC.adam_multi_members(count, big)):
            runs.append((cid, SC.adam_inputs(n, False, seed=1000 * count + i), lr, wd, step, 1.0))
    lr, wd, step = SC.PLANES_HYPER
    n = sum(r * c for r, c in SC.PLANES_SHAPES) + sum(SC.PLANES_GAPS)
    runs.append(("planes", SC.adam_inputs(n, False, seed=3), lr, wd, step, 1.0))
    return runs


def test_adamw_reference_is_torch_optim_adamw_in_float64():
    for n, (lr, wd, step0, zero) in [(37, SC.ADAM_HYPER["step1-zero-state"]), (37, SC.ADAM_HYPER["step2-lr5e-2-wd0"])]:
        p, m, v, gs = SC.adam_inputs(n, zero, seed=11)
        g3 = gs[0] * 0.5 + gs[1]
        param = torch.nn.Parameter(p.double().clone())
        opt = torch.optim.AdamW([param], lr=lr, betas=(SC.BETA1, SC.BETA2), eps=SC.EPS, weight_decay=wd)
        if step0 > 1 or not zero:  # start torch's state where the case starts
            opt.state[param] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m.double().clone(),
                                "exp_avg_sq": v.double().clone()}
        rp, rm, rv = p.double(), m.double(), v.double()
        for k, g in enumerate(list(gs) + [g3]):  # several steps
            param.grad = g.double().clone()
            opt.step()
            rp, rm, rv = SC.adamw_ref(rp, g, rm, rv, lr, wd, step0 + k)
            st = opt.state[param]
            assert torch.allclose(param.detach(), rp, rtol=1e-13, atol=1e-300), (n, k)
            assert torch.allclose(st["exp_avg"], rm, rtol=1e-13, atol=1e-300)
            assert torch.allclose(st["exp_avg_sq"], rv, rtol=1e-13, atol=1e-300)


def test_adamw_grad_scale_is_a_factor_on_the_gradient():
    p, m, v, (g, _) = SC.adam_inputs(50, False, seed=4)
    a = SC.adamw_ref(p, g, m, v, 1e-3, 1e-2, 7, grad_scale=1.0 / 1024)
    b = SC.adamw_ref(p, g.double() / 1024, m, v, 1e-3, 1e-2, 7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_adamw_fp32_restatement_error_is_the_recorded_one():
    worst = {k: 0.0 for k in SC.ADAM_F32_ERR}
    for cid, (p, m, v, gs), lr, wd, step, gscale in adam_case_steps():
        for k, g in enumerate(gs):
            ref = SC.adamw_ref(p, g, m, v, lr, wd, step + k, gscale)
            got = SC.adamw_f32(p, g, m, v, lr, wd, step + k, gscale)
            for name, e in SC.adam_errors(got, ref, p, m, g, lr, gscale).items():
                worst[name] = max(worst[name], e)
            p, m, v = got
    print("adamw fp32 restatement, largest errors:", {k: round(x, 4) for k, x in worst.items()})
    for name, rec in SC.ADAM_F32_ERR.items():
        assert rec / 1.25 <= worst[name] <= rec, (name, worst[name], rec)


def test_adamw_pinned_restatement_stays_inside_the_recorded_fp32_error():
    """The sequence the kernels pin (SC.adamw_pinned: exact arithmetic, one rounding per line) has fewer roundings than adamw_f32, so
    it stays inside adamw_f32's recorded error against float64; and the fmas make a difference -- it is not adamw_f32's bits."""
    differs = False
    for gscale in (1.0, 0.3):
        p, m, v, gs = SC.pinned_inputs(seed=64)
        for k, g in enumerate(gs):
            ref = SC.adamw_ref(p, g, m, v, 1e-3, 1e-2, 3 + k, gscale)
            got = SC.adamw_pinned(p, g, m, v, 1e-3, 1e-2, 3 + k, gscale)
            errs = SC.adam_errors(got, ref, p, m, g, 1e-3, gscale)
            print("adamw pinned restatement, grad_scale", gscale, "step", 3 + k, {n: round(e, 4) for n, e in errs.items()})
            for name, e in errs.items():
                assert e <= SC.ADAM_F32_ERR[name], (gscale, k, name, e)
            differs = differs or any(not torch.equal(a, b) for a, b in zip(got, SC.adamw_f32(p, g, m, v, 1e-3, 1e-2, 3 + k, gscale)))
            p, m, v = got
    assert differs


def test_round32_is_round_to_nearest_even_float32():
    from fractions import Fraction
    tie = Fraction(1) + Fraction(1, 2 ** 24)  # halfway between 1 and 1 + 2^-23: to even, 1
    assert SC._round32(tie) == 1 and SC._round32(tie + Fraction(1, 2 ** 60)) == 1 + Fraction(1, 2 ** 23)
    assert SC._round32(Fraction(3, 2 ** 150)) == Fraction(1, 2 ** 148)  # 1.5 denormal quanta: to even, 2 of them
    for x in (0.1, -2.5e-3, 3.4e38, 1e-40, 0.3):
        assert float(SC._round32(Fraction(x))) == float(torch.tensor(x, dtype=torch.float32)), x


def test_adam_inputs_plant_the_edge_elements():
    p, m, v, (g1, g2) = SC.adam_inputs(4097, False, seed=4097)
    assert g1[0] == 0 and g1[-1] == 0 and m[1] == 0 and v[1] == 0 and abs(p[3]) == 1e4 and abs(p[-4]) == 1e4
    assert g1[2] == 1e-20 and float(g1[2]) ** 2 < 2.0 ** -126 and (g1[2] * g1[2]).item() < 2.0 ** -126  # the square underflows
    # every third member of a multi case is unaligned, the big member is not, and it is past the per-tensor block cap
    mem = SC.adam_multi_members(49, 10)
    assert [s for _, s in mem[:6]] == [0, 0, 1, 0, 0, 1] and mem[10] == (SC.ADAM_MULTI_BIG, 0)
    assert (SC.ADAM_MULTI_BIG + 3) // 4 > 1024 * 256 and 49 > 48


def test_view_layout_alignment_and_guards():
    offs, total = SC.view_layout([(5, 0), (5, 1), (1, 0), (4097, 1)])
    ends = [o + n for o, n in zip(offs, (5, 5, 1, 4097))]
    assert [o % 4 for o in offs] == [0, 1, 0, 1]
    assert offs[0] >= SC.GUARD and all(b - a >= SC.GUARD for a, b in zip(ends, offs[1:])) and total - ends[-1] >= SC.GUARD
    g = SC.guard_mask(total, offs, (5, 5, 1, 4097))
    assert int((~g).sum()) == 5 + 5 + 1 + 4097


def test_bf16_rounding_reference_is_tensor_to_bfloat16():
    x = torch.cat([SC.planted_f32(4096, seed=1), torch.randn(4096, generator=SC.gen(2)) * 1e-39,
                   torch.randn(4096, generator=SC.gen(3)) * 1e38])
    # every 16-bit pattern with the tie pattern and its neighbours below it
    hi = torch.arange(0, 1 << 16, dtype=torch.int64)
    for low in (0x7FFF, 0x8000, 0x8001):
        x = torch.cat([x, torch.from_numpy(((hi << 16) | low).numpy().astype(np.uint32).view(np.float32).copy())])
    assert SC.same_bf16(SC.bf16_round_ref(x), x.to(torch.bfloat16))
    want = SC.bf16_round_ref(torch.tensor(SC.PLANTED[:9], dtype=torch.float32)).float().tolist()
    assert want == [1.0, 1.015625, -1.0, 0.0, -0.0, float("inf"), -float("inf"), float("inf"), -float("inf")]
    assert SC.bf16_round_ref(torch.tensor([1.5 * 2.0 ** -133, 1e-45])).float().tolist() == [2.0 ** -132, 0.0]


def test_reduce_reference_sums_in_rank_order_and_rounds_once():
    for W, chunk, scale in SC.REDUCE_CASES[:-1]:
        recv = SC.reduce_inputs(W, chunk, seed=W)
        acc = np.zeros(chunk, np.float32)
        for r in range(W):
            acc = (acc + recv[r * chunk:(r + 1) * chunk].float().numpy()).astype(np.float32)
        want = torch.from_numpy(acc * np.float32(scale)).to(torch.bfloat16)
        assert SC.same_bf16(SC.reduce_ref(recv, W, chunk, scale), want)
    assert all(c % 8 == 0 for _, c, _ in SC.REDUCE_CASES) and SC.REDUCE_CASES[-1][1] // 8 > SC.STREAM_GRID8


def test_prompt_mix_reference_is_the_einsum_of_test_prompt_mix():
    NL, NI, B, Lp, W = 3, 2, 2, 2, 8
    hid, n = W // 2, NI * B
    enc, _, gk, _ = SC.mix_inputs(NL, NI, B, Lp, W)
    wp, bp = torch.randn(NL * 4, Lp * W, generator=SC.gen(2)).double(), torch.randn(NL * 4, generator=SC.gen(3)).double()
    e = enc.double().requires_grad_(True)
    sm = e.view(NI, B, Lp, 4, W).mean(3).reshape(n, Lp * W)
    z = F.linear(sm, wp, bp)
    gate = torch.softmax(F.leaky_relu(z).view(n, NL, 4), -1)
    kv = torch.einsum("nik,nlkc->nilc", gate, e.view(n, Lp, 4, W))
    kv = kv.view(NI, B, NL, Lp, W).permute(2, 1, 0, 3, 4).reshape(NL, B, NI * Lp, W)
    ref = torch.stack([kv[..., :hid].reshape(NL, B, -1), kv[..., hid:].reshape(NL, B, -1)], 1)
    (ref * gk.double()).sum().backward()
    # the same through mix_ref, the Linear's backward applied by hand: dsm = dlogits . Wp
    dsm0 = torch.zeros(n, Lp * W)
    _, _, _, dz, _ = SC.mix_ref(enc, z.detach(), gk, dsm0, NL, NI, B, Lp, W)
    sm2, gate2, pkv2, dz2, denc2 = SC.mix_ref(enc, z.detach(), gk, dz @ wp, NL, NI, B, Lp, W)
    assert torch.allclose(pkv2, ref.detach(), rtol=1e-13) and torch.allclose(sm2, sm.detach(), rtol=1e-13)
    assert torch.allclose(gate2, gate.detach().reshape(n, NL * 4), rtol=1e-13)
    assert torch.allclose(denc2, e.grad, rtol=1e-11, atol=1e-13)
    # explicit loops for one output element and the split mean
    i, b, l, idx, c = 1, 1, 1, 2, 5
    nn_ = i * B + b
    want = sum(float(gate2[nn_, idx * 4 + k]) * float(enc[i, b, l, k * W + c]) for k in range(4))
    assert abs(float(pkv2[idx, 1, b, (i * Lp + l) * hid + c - hid]) - want) < 1e-12
    assert torch.allclose(SC.split_mean_ref(enc.reshape(-1), n * Lp, W), sm2.reshape(n * Lp, W), rtol=1e-13)


def test_mix_cases_cover_every_dispatched_depth_and_both_launch_geometries():
    assert sorted({c[0] for c in SC.MIX_CASES}) == SC.MIX_DEPTHS
    ids = [SC.mix_id(c) for c in SC.MIX_CASES]
    assert len(set(ids)) == len(ids)
    assert any("W264-256-thread-fallback" in i for i in ids) and any("W3072-256-thread-fallback-wraps" in i for i in ids)
    assert any("W1536-block384" in i for i in ids) and any("W256-block64" in i for i in ids)
    for NL, NI, B, Lp, W in SC.MIX_CASES:
        _, z, _, _ = SC.mix_inputs(NL, NI, B, Lp, W)
        assert z[0, 1] == 0 and float(z[-1, 2:].max()) <= -100


def test_mix_fp32_restatement_has_headroom():
    for c in SC.MIX_CASES:
        ins = SC.mix_inputs(*c)
        sm, gate, pkv, dz, denc = SC.mix_ref(*ins, *c)
        sm32, gate32, pkv32, dz32, denc32 = SC.mix_ref(*ins, *c, dtype=torch.float32)
        assert SC.close_excess(sm32, sm, SC.RTOL_SPLIT_MEAN) <= HEADROOM, c
        assert SC.close_excess(pkv32, pkv, SC.RTOL_MIX_FWD) <= HEADROOM, c
        assert SC.close_excess(dz32, dz, SC.RTOL_MIX_GRAD) <= HEADROOM, c
        assert SC.close_excess(denc32, denc, SC.RTOL_MIX_GRAD) <= HEADROOM, c
        assert SC.norm_excess(gate32, gate, SC.RTOL_GATE) <= HEADROOM, c


def test_split_mean_and_mean_l_fp32_restatements_have_headroom():
    for rows, W in SC.SPLIT_MEAN_CASES:
        enc = torch.randn(rows * 4 * W, generator=SC.gen(rows))
        e = enc.view(rows, 4, W)
        got = (e[:, 0] + e[:, 1] + e[:, 2] + e[:, 3]) * 0.25
        assert SC.close_excess(got, SC.split_mean_ref(enc, rows, W), SC.RTOL_SPLIT_MEAN) <= HEADROOM
    for n, L, W4 in SC.MEAN_L_CASES:
        enc, dmean, prior = SC.mean_l_inputs(n, L, W4)
        acc = torch.zeros(n, W4)
        for l in range(L):
            acc = acc + enc[:, l]
        inv = torch.tensor(1.0, dtype=torch.float32) / L
        assert SC.norm_excess(acc * inv, enc.double().mean(1), SC.RTOL_MEAN_L) <= HEADROOM, (n, L, W4)
        want = prior.double() + dmean.double()[:, None, :] / L
        assert SC.norm_excess(prior + dmean[:, None, :] * inv, want, SC.RTOL_MEAN_L) <= HEADROOM, (n, L, W4)


def test_gate_reference_and_fp32_headroom():
    for ng in SC.GATE_GROUPS:
        for mode in SC.GATE_MODES:
            z = SC.gate_logits(ng, mode)
            ref = SC.gate_ref(z)
            lz = torch.where(z.double() > 0, z.double(), 0.01 * z.double())
            loop = torch.stack([torch.exp(r - r.max()) / torch.exp(r - r.max()).sum() for r in lz])
            assert torch.allclose(ref, loop, rtol=1e-13, atol=1e-300)
            z32 = torch.where(z > 0, z, 0.01 * z)
            e = torch.exp(z32 - z32.max(-1, keepdim=True).values)
            got = e * (1.0 / e.sum(-1, keepdim=True))
            assert SC.norm_excess(got, ref, SC.RTOL_GATE) <= HEADROOM, (ng, mode)
            assert float((got.double().sum(-1) - 1).abs().max()) <= SC.GATE_SUM_TOL
            if mode in ("all-equal", "minus1e4-constant"):
                assert torch.equal(ref, torch.full_like(ref, 0.25)) and torch.equal(got, torch.full_like(got, 0.25))


def test_kl_reference_is_kl_div_of_log_softmax_and_fp32_has_headroom():
    kinds = set()
    for B, N in SC.KL_SHAPES:
        for mode in SC.KL_LOGITS:
            z, t = SC.kl_inputs(B, N, mode)
            kinds |= {SC.KL_TARGET_KINDS[(r + N) % 5] for r in range(B)}
            loss, dz = SC.kl_ref(z, t)
            # an independent statement: explicit sums, and the closed-form gradient with sum(target)
            zd, td = z.double(), t.double()
            lp = zd - zd.max(-1, keepdim=True).values
            lp = lp - lp.exp().sum(-1, keepdim=True).log()
            terms = torch.where(td > 0, td * (td.clamp_min(1e-300).log() - lp), torch.zeros_like(td))
            assert abs(float(terms.sum() / B) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
            grad = SC.KL_GOUT * SC.KL_GSCALE / B * (lp.exp() * td.sum(-1, keepdim=True) - td)
            assert torch.allclose(dz, grad, rtol=1e-9, atol=1e-15)
            for r in range(B):
                if SC.KL_TARGET_KINDS[(r + N) % 5] == "all-zero":
                    assert float(terms[r].sum()) == 0.0 and not bool(dz[r].any())
            loss32, dz32 = SC.kl_ref(z, t, dtype=torch.float32)
            assert SC.close_excess(loss32.reshape(1), loss.reshape(1), SC.RTOL_KL_LOSS) <= HEADROOM, (B, N, mode)
            assert SC.close_excess(dz32, dz, SC.RTOL_KL_GRAD, SC.ATOL_KL_GRAD) <= HEADROOM, (B, N, mode)
    assert kinds == set(SC.KL_TARGET_KINDS)
    z, t = SC.kl_inputs(5, 2089, "scale2")
    assert abs(float(t[(4 - 2089) % 5].sum()) - 0.5) < 1e-6  # the un-normalised row


def test_packing_reference_is_nonzero_and_a_stable_sort():
    for cid, B, S, P, kind, masked, pm in SC.PACK_MASK_CASES:
        m = SC.packing_mask(B, S, P, kind, masked, pm)
        assert m.shape == (B, P + S)
        keep = m[:, P:] > -5000
        cu, inv, rowmap, mv = SC.packing_ref(m, P, S)
        nz = keep.nonzero()
        flat = (nz[:, 0] * S + nz[:, 1]).int()
        assert mv == len(flat) and np.array_equal(rowmap[:mv], flat.numpy()) and (rowmap[mv:] == -1).all()
        assert np.array_equal(cu, np.concatenate([[0], keep.sum(1).cumsum(0).numpy()]))
        for r in range(mv):
            assert inv[rowmap[r]] == r
        assert (inv[~keep.reshape(-1).numpy()] == -1).all()
        cuo, invo, rowo, mvo = SC.packing_ref(m, P, S, ordered=True)
        order = torch.sort(keep.sum(1), descending=True, stable=True).indices
        assert cuo[0] == -1 and np.array_equal(cuo[1:B + 1], cu[1:]) and np.array_equal(cuo[B + 1:], order.numpy())
        assert np.array_equal(invo, inv) and np.array_equal(rowo, rowmap) and mvo == mv
        if pm:  # masked prefix columns do not matter
            m2 = m.clone()
            m2[:, :P] = 0
            assert all(np.array_equal(a, b) for a, b in zip(SC.packing_ref(m2, P, S)[:3], (cu, inv, rowmap)))
    kinds = [c[4] for c in SC.PACK_MASK_CASES]
    assert {"all", "none", "ragged", "holes", "ragged-one-empty"} <= set(kinds)
    assert any(c[1] > 16 for c in SC.PACK_MASK_CASES) and any(c[5] == -float("inf") for c in SC.PACK_MASK_CASES)


def test_ktile_reference_is_a_python_loop():
    counts = set()
    for bk, B, S in SC.KTILE_SHAPES:
        for pattern in SC.KTILE_PATTERNS:
            m = SC.ktile_mask(bk, B, S, pattern)
            live, cnt = SC.ktiles_ref(m, SC.KTILE_P, S, bk)
            want = []
            for t in range(B * S // bk):
                if any(float(m[r // S, SC.KTILE_P + r % S]) > -5000 for r in range(t * bk, (t + 1) * bk)):
                    want.append(t)
            assert list(live) == want and cnt == len(want)
            nt = B * S // bk
            counts.add(nt)
            if pattern == "nothing-live":
                assert cnt == 0
            if pattern == "one-tile-live-in-its-last-row-only":
                assert want == [nt // 2]
            if pattern == "dead-start-middle-end":
                assert not ({0, nt // 2, nt - 1} & set(want))
    assert {63, 64, 65} <= counts and any(S % bk for bk, _, S in SC.KTILE_SHAPES)


def test_gather_reference_is_a_row_loop():
    for rows, H in SC.GATHER_CASES[:3]:
        for kind in SC.GATHER_MAPS:
            src, mp = SC.gather_inputs(rows, H, kind)
            want = torch.stack([src[int(s)] if s >= 0 else torch.zeros(H) for s in mp])
            assert torch.equal(SC.gather_ref(src, mp), want)
    _, mp = SC.gather_inputs(128, 8, SC.GATHER_MAPS[0])
    assert int((mp < 0).sum()) > 0 and len(set(mp.tolist())) < 128
    rows, H = SC.GATHER_CASES[-1]
    assert rows * (H // 4) > 4096 * 256


def test_colsum_fp32_restatement_has_headroom():
    shapes = [(r, c, None) for r in SC.COLSUM_ROWS for c in SC.COLSUM_COLS] + list(SC.COLSUM_STRIDED) + \
             [(r, c, None) for r in SC.COLSUM_SMALL_ROWS for c in SC.COLSUM_SMALL_COLS]
    for rows, cols, ld in shapes:
        x, prior = SC.colsum_inputs(rows, cols, ld)
        for acc in (False, True):
            ref = x[:, :cols].double().sum(0) + (prior.double() if acc else 0)
            got = torch.zeros(cols)
            for r in range(0, rows, 64):  # a plain fp32 sum in row order, blocked only to keep the loop short
                got = got + x[r:r + 64, :cols].sum(0)
            got = got + prior if acc else got
            assert SC.close_excess(got, ref, SC.RTOL_COLSUM) <= HEADROOM, (rows, cols, ld, acc)


def test_dropout_conditions():
    for p in SC.DROPOUT_PS:
        # (1.f / (1.f - p) in fp32 is NOT this at p = 0.9: 9.999998, which is why mtvaf_dropout takes p as a double)
        assert SC.dropout_scale(p) == np.float32(1.0 / (1.0 - p)), p
        assert 0 < SC.keep_fraction_bound(p, SC.DROPOUT_N // 4) < 0.01
    assert SC.DROPOUT_STRIDE_N // 4 > 2048 * 256 and SC.DROPOUT_STRIDE_N % 4 == 0


def test_capped_grids_get_a_second_stride_trip():
    """the largest case of every grid-strided kernel is past its cap (blocks x 256 lanes x vector width)"""
    assert (SC.ADAM_CASES[-1][1] + 3) // 4 > 2048 * 256
    assert (SC.PACK_CASES[-1][0] + 7) // 8 > SC.STREAM_GRID8
    assert SC.SPLIT_MEAN_CASES[-1][0] * (SC.SPLIT_MEAN_CASES[-1][1] // 4) > 2048 * 256
    n, L, W4 = SC.MEAN_L_CASES[-1]
    assert n * (W4 // 4) > 2048 * 256 and n * L * (W4 // 4) > 2048 * 256
    assert SC.ZERO_SIZES[-1] // 4 > 4096 * 256
    assert SC.split_mean_id(SC.SPLIT_MEAN_CASES[-1]).endswith("stride-loop") and SC.mean_l_id(SC.MEAN_L_CASES[-1]).endswith("stride-loop")
