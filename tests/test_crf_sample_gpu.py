"""Posterior sampling and minimum-risk training on the MI355X: `mtvaf_crf_sample` / `CRF.sample` / `CRF.minimum_risk` /
`TVNetSAModel2` with ``args.crf_mrt_weight`` against the float64 references of tests/crf_sample_cases.py.  Tags on gapped uniforms
are compared exactly; scores, log-probabilities, risks and gradients by the bounds of crf_nbest_cases / crf_llh_cases, each printed
as err / bound before it is asserted."""
import numpy as np
import pytest
import torch

import crf_llh_cases as L
import crf_sample_cases as X
import params as P
import test_crf_entities_gpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda c: "C{}-S{}-K{}-B{}".format(*c[:4])  # noqa: E731


def crf_of(inp, batch_first=True):
    crf = T.make_crf(inp.start, inp.end, inp.trans)
    crf.batch_first = batch_first
    return crf


def sample_injected(case, **kw):
    ref = X.reference(case)
    out = crf_of(ref.inp).sample(ref.inp.em.to(DEV), ref.inp.mask.to(DEV), n_samples=case[2], uniforms=ref.u.to(DEV), **kw)
    return ref, out


# ---- 1. injected uniforms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_tags_scores_and_logprob_on_gapped_uniforms(case):
    from mtvaf_amd import engine
    offset = engine.RNG.offset
    ref, out = sample_injected(case, return_uniforms=True)
    assert engine.RNG.offset == offset  # injected uniforms leave the generator alone
    tags = out["tags"].cpu().numpy()
    assert out["tags"].dtype == torch.int32 and tags.shape == ref.tags.shape
    assert tags.tolist() == ref.tags.tolist()  # every draw of every sample, and -1 behind the length
    assert torch.equal(out["uniforms"].cpu(), ref.u)
    scores, logprob = out["scores"].double().cpu().numpy(), out["logprob"].double().cpu().numpy()
    worst_s = worst_p = 0.0
    for b in range(case[3]):
        err_s = float(np.abs(scores[b] - ref.scores[b]).max())
        err_p = float(np.abs(logprob[b] - (ref.scores[b] - ref.logz[b])).max())
        worst_s, worst_p = max(worst_s, err_s / ref.delta[b]), max(worst_p, err_p / (ref.delta[b] + ref.logz_bound))
    print(f"crf-sample {case}: score err / bound {worst_s:.4f}, logprob err / bound {worst_p:.4f}")
    assert worst_s <= 1.0 and worst_p <= 1.0
    assert (logprob <= ref.delta.max() + ref.logz_bound).all()  # a log probability


def test_every_output_element_is_overwritten_and_batch_first_false_is_the_same():
    from mtvaf_amd import hip
    case = (13, 16, 8, 5, 1321)
    ref, want = sample_injected(case, return_uniforms=True)
    C, S, K, B, _ = case
    crf = crf_of(ref.inp)
    junk = (torch.full((B, K, S), 77, dtype=torch.int32, device=DEV), torch.full((B, K), float("nan"), device=DEV),
            torch.full((B, K), float("nan"), device=DEV), torch.full((B, K, S), float("nan"), device=DEV))
    hip.crf_sample(ref.inp.em.to(DEV), ref.inp.mask.to(DEV), crf.start_transitions.data, crf.end_transitions.data,
                   crf.transitions.data, K, ref.u.to(DEV), out=junk)
    for got, k in zip(junk, ("tags", "scores", "logprob", "uniforms")):
        assert torch.equal(got, want[k]), k
    # without the optional outputs the others are the same bits
    lean = crf.sample(ref.inp.em.to(DEV), ref.inp.mask.to(DEV), n_samples=K, uniforms=ref.u.to(DEV), return_logprob=False)
    assert lean["logprob"] is None and "uniforms" not in lean
    assert torch.equal(lean["tags"], want["tags"]) and torch.equal(lean["scores"], want["scores"])
    # sequence-first emissions and mask; uniforms and every result stay batch-first
    seq = crf_of(ref.inp, batch_first=False).sample(ref.inp.em.to(DEV).transpose(0, 1), ref.inp.mask.to(DEV).transpose(0, 1),
                                                    n_samples=K, uniforms=ref.u.to(DEV), return_uniforms=True)
    for k in ("tags", "scores", "logprob", "uniforms"):
        assert torch.equal(seq[k], want[k]), k


def test_shapes_beyond_the_limits_are_errors():
    from mtvaf_amd import hip
    ref = X.reference((3, 4, 64, 5, 309))
    crf, em, mask = crf_of(ref.inp), ref.inp.em.to(DEV), ref.inp.mask.to(DEV)
    with pytest.raises(ValueError, match="n_samples=65"):
        crf.sample(em, mask, n_samples=65)
    with pytest.raises(ValueError, match="n_samples=0"):
        crf.sample(em, mask, n_samples=0)
    with pytest.raises(ValueError, match="uniforms"):
        crf.sample(em, mask, n_samples=4, uniforms=torch.zeros(5, 3, 4, device=DEV))
    lib = hip.lib()
    assert lib.mtvaf_crf_sample_workspace_bytes(5, 4, 3, 65) == 0 and lib.mtvaf_crf_sample_workspace_bytes(5, 513, 3, 8) == 0
    assert lib.mtvaf_crf_sample_workspace_bytes(5, 4, 65, 8) == 0 and lib.mtvaf_crf_sample_workspace_bytes(5, 4, 3, 64) > 0
    tags, sc = torch.full((5, 64, 4), 77, dtype=torch.int32, device=DEV), torch.zeros(5, 64, device=DEV)
    ws = torch.empty(lib.mtvaf_crf_sample_workspace_bytes(5, 4, 3, 64), dtype=torch.uint8, device=DEV)
    p = [em.data_ptr(), mask.data_ptr(), crf.start_transitions.data_ptr(), crf.end_transitions.data_ptr(), crf.transitions.data_ptr()]
    call = lambda K, wsb: lib.mtvaf_crf_sample(*p, K, None, 1, 2, tags.data_ptr(), sc.data_ptr(), None, None, 5, 4, 3,  # noqa: E731
                                               ws.data_ptr(), wsb, None)
    assert call(65, ws.numel()) == -1 and call(0, ws.numel()) == -1 and call(64, ws.numel() - 1) == -4
    torch.cuda.synchronize()
    assert (tags == 77).all()


# ---- 2. the generator ----------------------------------------------------------------------------------------------------------
def test_generator_mode():
    from mtvaf_amd import engine
    case = (17, 17, 5, 5, 1722)
    ref = X.reference(case)
    crf, em, mask = crf_of(ref.inp), ref.inp.em.to(DEV), ref.inp.mask.to(DEV)
    torch.manual_seed(31)
    engine.RNG.offset = 500
    a = crf.sample(em, mask, n_samples=5, return_uniforms=True)
    assert engine.RNG.offset == 501  # one offset per call
    b = crf.sample(em, mask, n_samples=5, return_uniforms=True)
    assert engine.RNG.offset == 502
    engine.RNG.offset = 500
    c = crf.sample(em, mask, n_samples=5, return_uniforms=True)
    u = a["uniforms"]
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    on = ref.inp.mask.bool()[:, None, :].expand(5, 5, 17).to(DEV)
    assert (u[~on] == 0).all() and (a["tags"][~on] == -1).all() and (a["tags"][on] >= 0).all() and (a["tags"][on] < 17).all()
    assert u[on].unique().numel() > 0.9 * int(on.sum())  # (b, k, t) each have a counter of their own
    for k in ("tags", "scores", "logprob", "uniforms"):
        assert torch.equal(a[k], c[k]), k              # the same (seed, offset): the same draw
    assert not torch.equal(a["uniforms"], b["uniforms"])  # another offset: another draw
    torch.manual_seed(32)
    engine.RNG.offset = 500
    assert not torch.equal(crf.sample(em, mask, n_samples=5, return_uniforms=True)["uniforms"], u)  # another seed
    fed = crf.sample(em, mask, n_samples=5, uniforms=u)
    for k in ("tags", "scores", "logprob"):
        assert torch.equal(fed[k], a[k]), k            # its uniforms handed back in: the same bits


def test_frequencies_follow_the_marginals():
    """One sentence (C = 5, len = 6) repeated B = 256 times at K = 16: 4096 draws, each with its own (b, k) counter.  The
    empirical p(y_t = j) lies within 5 sqrt(p (1 - p) / 4096) + 1e-3 of CRF.marginals; a pure function of the seed."""
    from mtvaf_amd import engine
    g = torch.Generator().manual_seed(77)
    em1 = torch.randn(1, 6, 5, generator=g) * 2
    inp = X.N.inputs((5, 6, 16, 1, 77))
    crf = crf_of(inp)
    em = em1.expand(256, 6, 5).contiguous().to(DEV)
    mask = torch.ones(256, 6, dtype=torch.uint8, device=DEV)
    torch.manual_seed(1234)
    engine.RNG.offset = 0
    tags = crf.sample(em, mask, n_samples=16, return_logprob=False)["tags"].long().reshape(4096, 6)
    freq = torch.nn.functional.one_hot(tags, 5).double().mean(0).cpu()   # [6,5]
    p = crf.marginals(em[:1], mask[:1])[0].double().cpu()
    tol = 5.0 * torch.sqrt(p * (1 - p) / 4096) + 1e-3
    q = float(((freq - p).abs() / tol).max())
    print(f"crf-sample frequencies: max |freq - p| / tolerance {q:.4f}")
    assert q <= 1.0
    assert tags.unique(dim=0).shape[0] > 50  # the draws differ


def test_graph_capture_replays_to_the_same_bits():
    ref, other = X.reference((13, 16, 8, 5, 1321)), X.inputs((13, 16, 8, 5, 1322))
    crf = crf_of(ref.inp)
    buf, mask_d, u = ref.inp.em.to(DEV).clone(), ref.inp.mask.to(DEV), ref.u.to(DEV)
    crf.sample(buf, mask_d, n_samples=8, uniforms=u)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crf.sample(buf, mask_d, n_samples=8, uniforms=u)
    seen = []
    for em in (ref.inp.em, other.em):
        buf.copy_(em)
        eager = crf.sample(buf, mask_d, n_samples=8, uniforms=u)
        graph.replay()
        for k in ("tags", "scores", "logprob"):
            assert torch.equal(out[k], eager[k]), k
        seen.append(out["tags"].cpu().clone())
    assert seen[0].numpy().tolist() == ref.tags.tolist() and not torch.equal(seen[0], seen[1])


# ---- 3. minimum risk -----------------------------------------------------------------------------------------------------------
def run_mrt(case, alpha, hyp=None, cost=None, reduction="none"):
    inp, h, c = X.mrt_inputs(case)
    hyp, cost = (h if hyp is None else hyp), (c if cost is None else cost)
    crf = crf_of(inp)
    em = inp.em.to(DEV).requires_grad_(True)
    risk = crf.minimum_risk(em, hyp.to(DEV), cost.to(DEV), mask=inp.mask.to(DEV), alpha=alpha, reduction=reduction)
    risk.sum().backward()
    return risk.detach(), dict(dem=em.grad, dstart=crf.start_transitions.grad, dend=crf.end_transitions.grad,
                               dtrans=crf.transitions.grad)


@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("case", X.MRT_CASES, ids=IDS)
def test_minimum_risk_forward(case, alpha):
    """costs in [0, 1]: the risk is 1-Lipschitz in alpha * llh, so it is held to alpha * bound("llh")"""
    ref = X.mrt_reference(case, alpha)
    risk, _ = run_mrt(case, alpha)
    err = float((risk.double().cpu() - ref.r64["risk"]).abs().max())
    bnd = alpha * ref.bound["llh"]
    print(f"crf-mrt {case} alpha {alpha}: risk err / bound {err / bnd:.4f} (err {err:.3e}, bound {bnd:.3e})")
    assert err <= bnd
    assert float(risk.min()) >= 0.0 and float(risk.max()) <= 1.0


@pytest.mark.parametrize("case", X.MRT_CASES, ids=IDS)
def test_minimum_risk_gradients(case):
    alpha = 1.0
    ref = X.mrt_reference(case, alpha)
    _, grads = run_mrt(case, alpha)
    worst = {}
    for k, g in grads.items():
        worst[k] = L.ratio(f"mrt-{k}", g, ref.r64[k], alpha * ref.bound[k])
    assert all(r <= 1.0 for r in worst.values()), worst
    assert float(ref.r64["dem"].abs().max()) > 1e-3  # the gradient is not trivially zero


def test_minimum_risk_reductions_duplicates_and_invalid_rows():
    case = X.MRT_CASES[0]
    inp, hyp, cost = X.mrt_inputs(case)
    base, gbase = run_mrt(case, 1.0)
    # a duplicated hypothesis (whatever its cost) and an invalid row change nothing
    more = torch.cat([hyp, hyp[:, 2:3], torch.full_like(hyp[:, :1], -1)], dim=1)
    more_cost = torch.cat([cost, cost[:, 2:3] + 0.5, torch.full_like(cost[:, :1], 0.9)], dim=1)
    risk, g = run_mrt(case, 1.0, more, more_cost)
    assert float((risk - base).abs().max()) <= 1e-6
    assert float((g["dem"] - gbase["dem"]).abs().max()) <= 1e-6 * max(1.0, float(gbase["dem"].abs().max()))
    # a sentence without a valid row: risk 0, zero gradient; the others are untouched
    bad = hyp.clone()
    bad[1] = -1
    risk, g = run_mrt(case, 1.0, bad)
    assert float(risk[1]) == 0.0 and float(g["dem"][1].abs().max()) == 0.0 and torch.isfinite(g["dem"]).all()
    assert torch.equal(risk[[0, 2, 3, 4]], base[[0, 2, 3, 4]])
    # a cost constant in k: that constant, and no gradient beyond rounding
    risk, g = run_mrt(case, 1.0, cost=torch.full_like(cost, 0.375))
    assert float((risk - 0.375).abs().max()) <= 1e-6 and float(g["dem"].abs().max()) <= 1e-6
    # reductions
    n_tok = float(inp.mask.sum())
    for red, want in (("sum", base.sum()), ("mean", base.mean()), ("token_mean", base.sum() / n_tok)):
        got, _ = run_mrt(case, 1.0, reduction=red)
        assert got.dim() == 0 and abs(float(got) - float(want)) <= 1e-6, red
    with pytest.raises(ValueError, match="reduction"):
        run_mrt(case, 1.0, reduction="median")


# ---- 4. the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [6, 32])  # 32 x 32 tokens: the Viterbi launch runs on the second stream
def test_model_with_crf_mrt_weight(B):
    from mtvaf_amd import engine
    S = 32
    cfg, plain = T.tiny_model(False)
    _, zero = T.tiny_model(False, crf_mrt_weight=0.0)
    _, mrt = T.tiny_model(False, crf_mrt_weight=0.5, crf_mrt_samples=6, crf_mrt_alpha=1.0)
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    labels[:, 0] = T.LABEL_MAP["[CLS]"]
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)

    def step(m, train=True):
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        m.zero_grad(set_to_none=True)
        out = m.train(train)(**kw)
        return out, engine.RNG.offset

    a, off_a = step(plain)
    z, off_z = step(zero)
    assert torch.equal(a.loss, z.loss) and list(a.logits) == list(z.logits) and off_a == off_z and zero.last_crf_mrt is None
    out, off = step(mrt)
    risk = mrt.last_crf_mrt
    assert off == off_a + 1 and list(out.logits) == list(a.logits)  # one offset for the samples, behind every dropout site
    assert risk.dim() == 0 and risk.is_cuda and not risk.requires_grad and 0.0 <= float(risk) <= 1.0
    assert torch.equal(out.loss.detach(), a.loss.detach() + 0.5 * risk)
    out.loss.backward()
    for name, p in mrt.named_parameters():
        if name.startswith(("fc.", "crf.", "bert.encoder.", "bert.embeddings.word")):
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    a.loss.backward()
    assert not torch.equal(mrt.fc.weight.grad, plain.fc.weight.grad)  # the term reaches the head
    # dropout off (eval mode), the same seed: the same bits
    first, _ = step(mrt, train=False)
    first, r1 = first.loss.detach().clone(), mrt.last_crf_mrt.clone()
    second, _ = step(mrt, train=False)
    assert torch.equal(first, second.loss.detach()) and torch.equal(r1, mrt.last_crf_mrt)
