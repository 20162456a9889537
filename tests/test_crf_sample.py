"""The references of the posterior-sampling and minimum-risk tests, checked against brute force on the CPU (no GPU): what
test_crf_sample_gpu.py compares the kernels with is itself exact."""
import numpy as np
import pytest
import torch

import crf_sample_cases as X


def tiny():
    """C = 3, one sentence of length 4 (the first of the (3, 4, 64, 5) case)"""
    inp = X.inputs((3, 4, 64, 5, 309))
    assert inp.lengths[0] == 4
    em, start, end, trans = (x.double().numpy() for x in (inp.em, inp.start, inp.end, inp.trans))
    return em[0], start, end, trans


def test_reference_sampler_partitions_the_unit_cube_by_the_path_distribution():
    """The sampler maps [0,1)^len onto paths; the volume that lands on a path must be its probability.  A column's cell
    boundaries depend only on the tag drawn behind it, so the volume of a path is the product over columns of the width of its
    tag's cell -- measured here by pushing the sampler through a stratified grid: per column the midpoints of the cells of ALL
    conditionals (every boundary any conditional has cuts the grid), weighted by the cell widths.  An exact partition by volume:
    1e-12."""
    em, start, end, trans = tiny()
    n, C = em.shape
    alpha = X.log_alphas(em, start, trans)
    grids = []
    for t in range(n):
        cuts = {0.0, 1.0}
        for y_next in range(C):
            w = X.weights(X.column(alpha, end, trans, t, y_next))
            cuts.update((np.cumsum(w)[:-1] / w.sum()).tolist())
        cuts = np.array(sorted(cuts))
        grids.append(((cuts[:-1] + cuts[1:]) / 2, np.diff(cuts)))
    paths, prob, _ = X.all_paths(em, start, end, trans)
    index = {tuple(p): i for i, p in enumerate(paths.tolist())}
    volume = np.zeros(len(paths))
    cells = np.array(np.meshgrid(*[np.arange(len(g[0])) for g in grids], indexing="ij")).reshape(n, -1).T
    for cell in cells:
        u = np.array([grids[t][0][c] for t, c in enumerate(cell)])
        vol = float(np.prod([grids[t][1][c] for t, c in enumerate(cell)]))
        volume[index[tuple(X.reference_sample(em, start, end, trans, u).tolist())]] += vol
    assert abs(volume.sum() - 1.0) < 1e-12
    assert np.abs(volume - prob).max() < 1e-12, np.abs(volume - prob).max()
    assert (prob > 0).all() and len(prob) == 81


def test_draw_rule_edges():
    x = np.log(np.array([0.25, 0.5, 0.25]))
    assert [X.draw(x, u) for u in (0.0, 0.2499, 0.25, 0.7499, 0.75, 0.9999)] == [0, 0, 1, 1, 2, 2]  # F_j > u F: a boundary goes up
    assert X.draw(x, 1.0) == 2                                          # no j: the highest tag with w > 0
    assert X.draw(np.array([0.0, -np.inf, 0.0, -np.inf]), 1.0) == 2     # ... which skips the weightless ones
    assert X.draw(np.array([-np.inf, 0.0, -np.inf]), 0.0) == 1          # a weightless tag is never drawn


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "C{}-S{}-K{}-B{}".format(*c[:4]))
def test_gapped_uniforms_construct(case):
    """Every draw of every case finds a gapped uniform within 64 redraws (make_reference raises otherwise); the batches are
    ragged and hold a sentence of length 1; the reference tags are the reference sampler's on those uniforms."""
    C, S, K, B, _ = case
    ref = X.reference(case)
    assert ref.inp.lengths[0] == S and (B == 1 or ref.inp.lengths[1] == 1)
    u = ref.u.numpy()
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    for b, n in enumerate(ref.inp.lengths):
        assert (ref.tags[b, :, n:] == -1).all() and (u[b, :, n:] == 0).all()
        for k in range(min(K, 3)):
            want = X.reference_sample(ref.em[b, :n], ref.start, ref.end, ref.trans, u[b, k, :n].astype(np.float64))
            assert ref.tags[b, k, :n].tolist() == want.tolist()
    print(f"crf-sample case {case}: centre {ref.inp.centre}, {ref.redraws} redraws")


def test_minimum_risk_over_all_paths_is_the_expected_cost():
    """With every path in the hypothesis set and alpha = 1 the renormalised weights are the posterior itself."""
    em, start, end, trans = tiny()
    paths, prob, _ = X.all_paths(em, start, end, trans)
    cost = torch.rand(1, len(paths), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    risk, llh = X.minimum_risk(t(em)[None], t(start), t(end), t(trans), torch.ones(1, 4, dtype=torch.uint8), t(paths)[None], cost)
    assert abs(float(risk[0]) - float((prob * cost[0].numpy()).sum())) < 1e-12
    assert np.abs(np.exp(llh[0].numpy()) - prob).max() < 1e-12
    # duplicates and invalid rows change nothing
    hyp = torch.cat([t(paths)[None], t(paths)[None, :5], torch.full((1, 2, 4), -1, dtype=torch.int64)], dim=1)
    cost2 = torch.cat([cost, cost[:, :5] + 7.0, torch.full((1, 2), 9.0, dtype=torch.float64)], dim=1)
    risk2, _ = X.minimum_risk(t(em)[None], t(start), t(end), t(trans), torch.ones(1, 4, dtype=torch.uint8), hyp, cost2)
    assert abs(float(risk2[0]) - float(risk[0])) < 1e-12


def test_constant_cost_gives_that_constant_and_no_gradient():
    case = X.MRT_CASES[0]
    inp, hyp, _ = X.mrt_inputs(case)
    r = X.mrt_oracle(case, 1.0, torch.float64, cost=torch.full(hyp.shape[:2], 0.375))
    assert float((r["risk"] - 0.375).abs().max()) < 1e-12
    for k in ("dem", "dstart", "dend", "dtrans"):
        assert float(r[k].abs().max()) < 1e-12, k
    # an all-invalid sentence: risk 0, nothing flows
    bad = hyp.clone()
    bad[1] = -1
    r = X.mrt_oracle(case, 1.0, torch.float64, hyp=bad)
    assert float(r["risk"][1]) == 0.0 and float(r["dem"][1].abs().max()) == 0.0
