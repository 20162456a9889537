"""The references and bounds of span_cases.py, proved on the host: the references on closed-form cases (S = 1, C = 1, uniform
scores, shift invariance, the index block by brute force), the builders against what their ids promise, and every bound --
inherited or derived -- against a plain fp32 restatement of the operation, which must stay within HEADROOM = 0.25 of it on
every case of the tables.  The restatement of the formula the loss kernels had before (sum pos z against den lse, m + log e -
z_label) must exceed the same bounds on the offset kinds from an offset of 1e4 on (at 1e3 what it loses is inside the inherited
tolerances, which are not narrowed): the tests tell the two forms apart.

test_fp32_restatements_keep_four_fold_headroom prints the largest host excess per bound."""
import math

import torch
import torch.nn.functional as F

import span_cases as SC
from oracle import mtvaf_oracle as O

HEADROOM = 0.25


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def test_index_ref_is_the_brute_force_walk():
    for c in SC.INDEX_CASES[2:]:
        mask, starts, ends = SC.index_inputs(c)
        B, S, M = c["B"], c["S"], c["M"]
        rowmap, fidx, woff, soff, width, run, jr = [], [], [], [], [], 0, 0
        for b in range(B):
            woff.append(run)
            for s in range(S):
                if int(mask[b, s]):
                    rowmap.append(b * S + s)
                    fidx.append(run)
                    run += 1
                else:
                    fidx.append(-1)
        for b in range(B):
            for m in range(M):
                soff.append(int(starts[b, m]) + woff[b])
                width.append(int(ends[b, m]) - int(starts[b, m]) + 1)
                jr = max(jr, width[-1])
        block, spec = SC.index_ref(mask, starts, ends)
        want = rowmap + [0] * (B * S - run) + fidx + woff + soff + width + [run, min(jr, S)]
        assert block.numel() == 2 * B * S + B + 2 * B * M + 2
        assert torch.equal(block[spec], torch.tensor(want, dtype=torch.int32)[spec]), c["id"]
        assert int(spec.logical_not().sum()) == B * S - run


def test_index_cases_reach_their_branches():
    by = {c["id"]: c for c in SC.INDEX_CASES}
    geo = lambda c: SC.span_geometry(*SC.index_inputs(c))
    c = SC.INDEX_CASES[0]
    assert c["B"] * c["S"] > SC.INDEX_THREADS and c["S"] % -(-c["B"] * c["S"] // SC.INDEX_THREADS) == 1
    assert SC.INDEX_CASES[1]["B"] * SC.INDEX_CASES[1]["M"] > SC.INDEX_THREADS
    mask, starts, ends = SC.index_inputs(by["B3-S7-M3-masked-sentence-between-live-ones"])
    assert not mask[1].any() and mask[0].any() and mask[2].any()
    assert geo(by["B2-S5-M2-T0-all-masked"])[4] == 0 and geo(by["B2-S5-M2-T1"])[4] == 1
    assert geo(by["B2-S6-M3-all-widths-nonpositive-JR0"])[5] == 0
    g = geo(by["B2-S6-M3-one-span-wider-than-S-JR-clamped"])
    assert g[5] == 6 and int(g[3].max()) > 6
    for c in SC.INDEX_CASES + SC.POOL_CASES + SC.POOL_ZERO_CASES:  # the contract: starts >= 0
        assert int((SC.pool_inputs(c)[2] if "H" in c else SC.index_inputs(c)[1]).min()) >= 0, c["id"]


def test_uniform_scores_pool_to_the_mean_of_the_span_rows():
    c = SC.POOL_CASES[0]
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(c)
    pooled, dseq, dw, db = SC.pool_ref(seq, mask, starts, ends, torch.zeros_like(wu), bu, gw)
    rowmap, _, soff, width, T, JR = SC.span_geometry(mask, starts, ends)
    flat = seq.double().reshape(-1, c["H"])[rowmap]
    for n in range(starts.numel()):
        rows = [min(int(soff[n]) + r, T - 1) for r in range(int(width[n]))]
        assert torch.allclose(pooled[n], flat[rows].mean(0), rtol=1e-12, atol=1e-14)
    assert float(db.abs().max()) <= 1e-12  # the softmax does not see the bias


def test_pool_cases_reach_their_branches():
    by = {c["id"]: c for c in SC.POOL_CASES}
    c = [c for c in SC.POOL_CASES if "130-spans" in c["id"]][0]
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(c)
    rowmap, _, soff, width, T, JR = SC.span_geometry(mask, starts, ends)
    covers = (soff <= 1) & (soff + JR - 1 >= 1)
    assert int(covers.sum()) == 130 and bool(covers[128:].any())  # a hit in every one of the three ballot rounds
    read = SC.rows_read(mask, starts, ends)
    assert int(mask.reshape(-1)[~read].sum()) >= 1 and int((mask == 0).sum()) >= 1  # a live row no span reads, a masked row
    c = [c for c in SC.POOL_CASES if "pile-onto" in c["id"]][0]
    _, mask, starts, ends = SC.pool_inputs(c)[:4]
    _, _, soff, _, T, JR = SC.span_geometry(mask, starts, ends)
    assert int((soff + JR - 1 > T - 1).sum()) >= 2
    assert {SC.pool_inputs(c)[2].numel() % 4 for c in SC.POOL_CASES} >= {1, 2, 3}
    for kind in ("ascending", "descending"):
        seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(by["B2-S6-M3-H8-score-" + kind])
        sc = (seq.double().reshape(-1, 8) @ wu.double().view(8) + bu.double())[mask.reshape(-1) != 0]
        d = sc[1:] - sc[:-1]
        assert bool((d > 0).all()) if kind == "ascending" else bool((d < 0).all())
    # "additive mask": a position behind its span, at -10000, still takes most of the weight of some span
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(by["B2-S6-M3-H8-score-addmask2e4"])
    emb, sm, score, _ = SC._pool_parts(seq, mask, starts, ends, wu, bu, torch.float64)
    p = torch.softmax(score.detach() + (1.0 - sm.double()) * SC.MASKED, -1)
    assert float((p * (~sm)).sum(-1).max()) > 0.5
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(by["B2-S6-M3-H8-score-onehot50"])
    assert 20 < float(SC._pool_parts(seq, mask, starts, ends, wu, bu, torch.float64)[2].detach().abs().max()) < 200


def test_truncating_a_span_wider_than_S_is_the_reference_at_JR_equal_S():
    c = [c for c in SC.POOL_CASES if "wider-than-S" in c["id"]][0]
    seq, mask, starts, ends, wu, bu, gw = SC.pool_inputs(c)
    cut = torch.minimum(ends, starts + c["S"] - 1)
    assert not torch.equal(cut, ends)
    a, b = SC.pool_ref(seq, mask, starts, ends, wu, bu, gw), SC.pool_ref(seq, mask, starts, cut, wu, bu, gw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert SC.span_geometry(mask, starts, ends)[5] == c["S"]


def test_distant_ce_closed_forms_and_shift_invariance():
    z, pos = SC.dce_inputs(SC.DCE_CASES[0])  # S = 1
    loss, dz = SC.dce_ref(z, pos, 0.5, 1.7)
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0
    c = [c for c in SC.DCE_CASES if c["logits"] == "plain" and c["S"] == 65][0]
    z, pos = SC.dce_inputs(c)
    l0, d0 = SC.dce_ref(z.double(), pos, 0.5, 1.7)
    for off in (1e3, -1e4):
        l1, d1 = SC.dce_ref(z.double() + off, pos, 0.5, 1.7)
        assert abs(float(l1 - l0)) <= 1e-10 * abs(float(l0)) and float((d1 - d0).abs().max()) <= 1e-10 * float(d0.abs().max())
    # the reference is the oracle's function, and a one-hot row is a row of F.cross_entropy
    hot = torch.zeros_like(pos)
    hot[torch.arange(pos.shape[0]), torch.arange(pos.shape[0])] = 1
    assert torch.allclose(O.distant_cross_entropy(z.double(), hot), F.cross_entropy(z.double(), torch.arange(pos.shape[0])), rtol=1e-13)
    z, pos = SC.dce_inputs(SC.DCE_EMPTY_ROW_CASE)
    loss, dz = SC.dce_ref(z, pos, 0.5, 1.7)
    r = SC.DCE_EMPTY_ROW_CASE["empty_row"]
    assert math.isnan(float(loss)) and bool(dz[r].isnan().all()) and not bool(dz[[0, 2]].isnan().any())


def test_ce_closed_forms_and_shift_invariance():
    z, lab = SC.ce_inputs(SC.CE_CASES[0])  # C = 1
    loss, dz, tot, cnt = SC.ce_ref(z, lab)
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and cnt == 5
    z, lab = SC.ce_inputs(SC.CE_CASES[3])
    assert int(lab[0]) == 63 and int(lab[1]) == 0
    l0, d0, t0, _ = SC.ce_ref(z.double(), lab)
    l1, d1, t1, _ = SC.ce_ref(z.double() - 1e4, lab)
    assert abs(float(l1 - l0)) <= 1e-10 * float(l0) and float((d1 - d0).abs().max()) <= 1e-10
    z, lab = SC.ce_inputs(SC.CE_ALL_IGNORED_CASE)
    loss, dz, tot, cnt = SC.ce_ref(z, lab)
    assert math.isnan(float(loss)) and cnt == 0 and float(tot) == 0.0 and not bool(dz.any())
    for c in SC.CE_CASES:  # the contract: labels in [0, C) or -100
        z, lab = SC.ce_inputs(c)
        assert bool(((lab == -100) | ((lab >= 0) & (lab < c["C"]))).all()), c["id"]
        if c["ignore"] == "every-third" and c["N"] > 2:
            assert bool((lab[2::3] == -100).all())


def test_mask_mul_cases():
    big = [s for s in SC.MASK_MUL_SHAPES if s[0] * s[1] * s[2] // 4 > SC.MASK_MUL_GRID4]
    assert big == [(3, 342, 4096)]
    x, row, col = SC.mask_mul_inputs(5, 33, 768, "both")
    scale = torch.tensor(1.0 / (1.0 - SC.MASK_MUL_P), dtype=torch.float32)
    assert set(row.tolist()) == set(col.reshape(-1).tolist()) == {0.0, 1.0, float(scale)}
    out = SC.mask_mul_ref(x, row, col)
    assert torch.equal(out, (x * row.view(5, 33, 1)) * col.view(5, 1, 768))
    assert SC.mask_mul_inputs(2, 1, 4, "row")[2] is None and SC.mask_mul_inputs(2, 1, 4, "col")[1] is None


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------------
def pool_excesses(c, got, ref=None):
    """excess of (pooled, dseq, dw, db) against the float64 reference under the case's bounds -> dict"""
    inp = SC.pool_inputs(c)
    ref = ref or SC.pool_ref(*inp)
    t = SC.pool_terms(*inp, cond=c["score"] in SC.POOL_COND_KINDS)
    return {"pooled": SC.excess(got[0], ref[0], SC.RTOL_POOLED, t["pooled"]),
            "dseq": SC.excess(got[1], ref[1], SC.RTOL_POOL_GRAD, t["dseq"]),
            "dw": SC.excess(got[2], ref[2], SC.RTOL_POOL_GRAD, t["dw"]),
            "db": SC.excess(got[3], ref[3], SC.RTOL_POOL_GRAD, t["db"])}


def test_fp32_restatements_keep_four_fold_headroom():
    worst = {}

    def note(k, v, cid):
        assert v <= HEADROOM, (k, cid, v)
        worst[k] = max(worst.get(k, 0.0), v)

    for c in SC.POOL_CASES:
        inp = SC.pool_inputs(c)
        for k, v in pool_excesses(c, SC.pool_ref(*inp, dtype=torch.float32)).items():
            note("pool " + k, v, c["id"])
    for c in SC.DCE_CASES:
        z, pos = SC.dce_inputs(c)
        rl, rd = SC.dce_ref(z, pos, c["scale"], c["gout"])
        for name, (l, d) in (("torch", SC.dce_ref(z, pos, c["scale"], c["gout"], dtype=torch.float32)),
                             ("lines", SC.dce_shift_safe_f32(z, pos, c["scale"], c["gout"]))):
            note("dce loss", SC.loss_excess(l, rl), c["id"] + name)
            note("dce dlogits", SC.excess(d, rd, SC.RTOL_DLOGITS), c["id"] + name)
    for c in SC.CE_CASES:
        z, lab = SC.ce_inputs(c)
        rl, rd, rt, cnt = SC.ce_ref(z, lab)
        l32, d32, _, _ = SC.ce_ref(z, lab, dtype=torch.float32)
        ll, lt = SC.ce_shift_safe_f32(z, lab)
        for name, l in (("torch", l32), ("lines", ll)):
            note("ce loss", SC.loss_excess(l, rl, SC.ce_sum_term(cnt, rl)), c["id"] + name)
        note("ce ws2", SC.loss_excess(lt, rt, SC.ce_sum_term(cnt, rt)), c["id"])
        note("ce dlogits", SC.excess(d32, rd, SC.RTOL_DLOGITS), c["id"])
    print({k: round(v, 4) for k, v in worst.items()})


def test_cancelling_formulas_exceed_the_bounds_on_the_offset_kinds():
    seen = {}
    for c in SC.DCE_CASES:
        if c["logits"] not in SC.DCE_OFFSET_KINDS:
            continue
        z, pos = SC.dce_inputs(c)
        rl, rd = SC.dce_ref(z, pos, c["scale"], c["gout"])
        l, d = SC.dce_cancelling_f32(z, pos, c["scale"], c["gout"])
        e = max(SC.loss_excess(l, rl), SC.excess(d, rd, SC.RTOL_DLOGITS))
        seen[c["logits"]] = max(seen.get(c["logits"], 0.0), e)
    print("distant-CE, cancelling form:", {k: round(v, 2) for k, v in seen.items()})
    # at +-1e3 the cancelling distant-CE form loses 6e-6 (loss) and 2e-5 (dlogits) relative: inside the inherited 1e-5 and 1e-4,
    # which are not narrowed here -- the bounds separate the two forms from 1e4 on
    assert len(seen) == 4 and seen["offset+1e4"] > 1 and seen["offset-1e4"] > 1, seen
    seen = {}
    for c in SC.CE_CASES:
        if c["logits"] not in SC.CE_OFFSET_KINDS:
            continue
        z, lab = SC.ce_inputs(c)
        rl, _, rt, cnt = SC.ce_ref(z, lab)
        l, t = SC.ce_cancelling_f32(z, lab)
        seen[c["logits"]] = max(seen.get(c["logits"], 0.0), SC.loss_excess(l, rl, SC.ce_sum_term(cnt, rl)))
    print("CE, cancelling form:", {k: round(v, 2) for k, v in seen.items()})
    # (a row loses up to ulp(1e3) / 2 = 3e-5 at +-1e3, but the signs are random and the mean over the rows stays inside 1e-5)
    assert len(seen) == 4 and seen["offset+1e4"] > 1 and seen["offset-1e4"] > 1, seen


def test_zero_cases_have_nothing_to_pool():
    for c in SC.POOL_ZERO_CASES:
        inp = SC.pool_inputs(c)
        T, JR = SC.span_geometry(*inp[1:4])[4:]
        assert T == 0 or JR == 0
        assert all(not bool(t.any()) for t in SC.pool_ref(*inp))
