"""The constrained CRF entry points (mtvaf_crf_lattice_{fwd,bwd,marginals,viterbi}) and the layers above them --
CRF.partial_llh / constrained_marginals / decode_constrained, TVNetSAModel2.predict_constrained and forward(allowed_tags=) --
on the MI355X, against the float64 references under the acceptance rule of crf_lattice_cases.

Largest err / bound per quantity over this file, one run on one MI355X: pllh 0.08, logz_a 0.34, logz
0.004, marg 0.009, dem 0.009, dstart 0.02, dend 0.03, dtrans 0.03, Viterbi score 0.04."""
import types

import pytest
import torch
from transformers import BertConfig

import crf_lattice_cases as X
import crf_llh_cases as L
import entity_cases as E
import params as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(s, p) for s in X.SHAPES for p in X.PATTERNS]


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _on(mask):
    return torch.arange(mask.shape[1])[None] < X.lengths_of(mask)[:, None]


def _fwd_bwd(hip, ref, accumulate, fill=(0.0, 0.0, 0.0)):
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    allowed, w = _dev(ref.allowed, ref.w)
    B, S, C = em.shape
    ws, wsb = hip.crf_lattice_workspace(B, S, C, DEV)
    pllh, logz_a, logz = (torch.full((B,), 7.0, device=DEV) for _ in range(3))
    hip.crf_lattice_fwd(em, allowed, mask, start, end, trans, pllh, logz_a, logz, ws, wsb)
    dem = torch.full((B, S, C), 7.0, device=DEV)
    ds, de, dt = torch.full((C,), fill[0], device=DEV), torch.full((C,), fill[1], device=DEV), torch.full((C, C), fill[2], device=DEV)
    hip.crf_lattice_bwd(w, em, allowed, mask, start, end, trans, dem, ds, de, dt, accumulate, ws, wsb)
    return dict(pllh=pllh, logz_a=logz_a, logz=logz, dem=dem, dstart=ds, dend=de, dtrans=dt)


# ---- 1. likelihood and gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pattern", CASES, ids=str)
def test_fwd_bwd_abi(hip, shape, pattern):
    """pllh, logz_a, logz; the backward with per-sentence weights of mixed sign (one an exact 0) accumulated onto prefilled
    parameter gradients, then overwriting; exact zeros at masked columns and for the zero-weight sentence."""
    ref = X.reference(shape, pattern)
    B = ref.inputs[0].shape[0]
    got = _fwd_bwd(hip, ref, True, fill=(0.5, -2.0, 3.0))
    for name in ("pllh", "logz_a", "logz", "dem"):
        X.check(ref, name, got[name])
    X.check(ref, "dstart", got["dstart"], add=0.5)
    X.check(ref, "dend", got["dend"], add=-2.0)
    X.check(ref, "dtrans", got["dtrans"], add=3.0)
    dem = got["dem"].cpu()
    assert bool((dem[~_on(ref.inputs[2])] == 0).all())
    if B >= 2:
        assert float(ref.w[1]) == 0.0 and bool((dem[1] == 0).all())
    over = _fwd_bwd(hip, ref, False, fill=(9.0, 9.0, 9.0))
    for name in ("dstart", "dend", "dtrans"):
        X.check(ref, name, over[name])
    if pattern in ("a", "e"):  # full sets: nothing is paid and nothing moves, exactly
        assert bool((got["pllh"] == 0).all()) and not bool(torch.signbit(got["pllh"]).any())
        for name in ("dem", "dstart", "dend", "dtrans"):
            assert bool((over[name] == 0).all()), name
    if pattern == "e":  # zero words and garbage above C are the full set, bit for bit
        same = _fwd_bwd(hip, X.reference(shape, "a"), False)
        for name in over:
            assert torch.equal(over[name], same[name]), name


@pytest.mark.parametrize("shape", X.SHAPES, ids=str)
def test_singletons_agree_with_the_log_likelihood(shape):
    """Pattern (b) through the module: partial_llh is CRF.forward(reduction='none') inside the rule."""
    from mtvaf_amd.modules.crf import CRF
    ref = X.reference(shape, "b")
    em, tags, mask, start, end, trans = _dev(*ref.inputs)
    crf = CRF(em.shape[2], batch_first=True).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start), crf.end_transitions.copy_(end), crf.transitions.copy_(trans)
    pllh, logz_a, logz = crf.partial_llh(em, ref.allowed.to(DEV), mask, return_parts=True)
    llh = crf(em, tags, mask=mask, reduction="none")
    X.check(ref, "pllh", pllh)
    X.check(ref, "pllh", llh)
    X.check(ref, "logz_a", logz_a)
    X.check(ref, "logz", logz)
    n = float(mask.sum())
    for red, want in (("sum", ref.r64["pllh"].sum()), ("mean", ref.r64["pllh"].mean()), ("token_mean", ref.r64["pllh"].sum() / n)):
        got = float(crf.partial_llh(em, ref.allowed.to(DEV), mask, reduction=red).detach())
        assert abs(got - float(want)) <= ref.bound["pllh"] * (em.shape[0] if red == "sum" else 1.0), red


def test_partial_llh_autograd_and_time_major_layout():
    from mtvaf_amd.modules.crf import CRF
    ref = X.reference((3, 17, 11, 1), "c")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    for batch_first in (True, False):
        crf = CRF(11, batch_first=batch_first).to(DEV)
        with torch.no_grad():
            crf.start_transitions.copy_(start), crf.end_transitions.copy_(end), crf.transitions.copy_(trans)
        e = (em if batch_first else em.transpose(0, 1)).clone().requires_grad_(True)
        a, m = ref.allowed.to(DEV), mask
        if not batch_first:
            a, m = a.t(), m.t()
        (crf.partial_llh(e, a, m) * ref.w.to(DEV)).sum().backward()
        X.check(ref, "dem", e.grad if batch_first else e.grad.transpose(0, 1))
        X.check(ref, "dstart", crf.start_transitions.grad)
        X.check(ref, "dend", crf.end_transitions.grad)
        X.check(ref, "dtrans", crf.transitions.grad)
        marg = crf.constrained_marginals(e.detach(), a, m)
        X.check(ref, "marg", marg if batch_first else marg.transpose(0, 1))


# ---- 2. constrained posteriors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pattern", CASES, ids=str)
def test_marginals_abi(hip, shape, pattern):
    ref = X.reference(shape, pattern)
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    B, S, C = em.shape
    ws, wsb = hip.crf_lattice_workspace(B, S, C, DEV)
    marg, logz_a = torch.full((B, S, C), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    hip.crf_lattice_marginals(em, ref.allowed.to(DEV), mask, start, end, trans, marg, logz_a, ws, wsb)
    X.check(ref, "marg", marg)
    X.check(ref, "logz_a", logz_a)
    m, on = marg.cpu(), _on(ref.inputs[2])
    assert bool((m[~on] == 0).all()) and bool((m[~ref.sets] == 0).all()) and float(m.min()) >= 0.0
    assert float((m.sum(-1)[on].double() - 1).abs().max()) <= ref.bound["marg"]
    marg2 = torch.full((B, S, C), 7.0, device=DEV)
    hip.crf_lattice_marginals(em, ref.allowed.to(DEV), mask, start, end, trans, marg2, None, ws, wsb)  # logz_a is optional
    assert torch.equal(marg2, marg)


# ---- 3. Viterbi --------------------------------------------------------------------------------------------------------------
def _decode(hip, inp, allowed):
    em, _, mask, start, end, trans = _dev(*inp)
    B, S, C = em.shape
    tags, lens = torch.full((B, S), 77, dtype=torch.int32, device=DEV), torch.full((B,), 77, dtype=torch.int32, device=DEV)
    score = torch.full((B,), 7.0, device=DEV)
    hip.crf_lattice_viterbi(em, allowed.to(DEV), mask, start, end, trans, tags, lens, score)
    return tags.cpu(), lens.cpu(), score.cpu()


@pytest.mark.parametrize("shape,pattern", CASES, ids=str)
def test_viterbi_abi(hip, shape, pattern):
    ref = X.reference(shape, pattern)
    inp = ref.inputs
    em, _, mask, start, end, trans = inp
    tags, lens, score = _decode(hip, inp, ref.allowed)
    n = X.lengths_of(mask)
    on = _on(mask)
    assert lens.tolist() == n.tolist() and bool((tags[~on] == -1).all())
    t = tags.long().clamp(min=0)
    assert bool((tags[on] >= 0).all()) and bool(ref.sets.gather(2, t[..., None])[..., 0][on].all()), "a tag outside its set"
    _, _, best64 = X.viterbi(em, ref.allowed, mask, start, end, trans)
    _, _, best32 = X.viterbi(em.float(), ref.allowed, mask, start.float(), end.float(), trans.float())
    own64 = X.path_score(em, tags, mask, start, end, trans)
    bnd = L.bound("logz", best64, best32)
    print(f"crf-lattice viterbi score {float((score.double() - own64).abs().max()) / bnd:.4f} "
          f"optimum {float((own64 - best64).abs().max()) / bnd:.4f} (bound {bnd:.3e})")
    assert bool(torch.isfinite(score).all())
    assert float((score.double() - own64).abs().max()) <= bnd
    assert float((own64 - best64).abs().max()) <= bnd
    if pattern in ("a", "e"):  # full sets: mtvaf_crf_viterbi's output, bit for bit
        d = _dev(*inp)
        t0, l0 = torch.empty_like(tags, device=DEV), torch.empty_like(lens, device=DEV)
        hip.crf_viterbi(d[0], d[2], d[3], d[4], d[5], t0, l0)
        assert torch.equal(t0.cpu(), tags) and torch.equal(l0.cpu(), lens)


@pytest.mark.parametrize("shape,pattern", CASES, ids=str)
def test_viterbi_tie_rule_on_exact_inputs(hip, shape, pattern):
    """Scores that are multiples of 1/8: float32 is exact, ties are frequent, so the tags are the float64 reference's."""
    inp = X.exact_inputs(shape)
    allowed, em = X.sets(shape, pattern, inp)
    inp = (em,) + inp[1:]
    tags, lens, score = _decode(hip, inp, allowed)
    want, n, best = X.viterbi(em, allowed, *inp[2:])
    assert torch.equal(tags.long(), want) and lens.tolist() == n.tolist()
    assert torch.equal(score.double(), best)


def test_decode_constrained_module(hip):
    from mtvaf_amd.modules.crf import CRF
    ref = X.reference((3, 65, 11, 1), "c")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    crf = CRF(11, batch_first=True).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start), crf.end_transitions.copy_(end), crf.transitions.copy_(trans)
    tags, lens, score = crf.decode_constrained(em, ref.allowed.to(DEV), mask, return_score=True)
    want = _decode(hip, ref.inputs, ref.allowed)
    assert torch.equal(tags.cpu(), want[0]) and torch.equal(lens.cpu(), want[1]) and torch.equal(score.cpu(), want[2])
    full = torch.zeros_like(ref.allowed).to(DEV)
    t1, l1 = crf.decode_constrained(em, full, mask)
    t0, l0 = crf.decode_packed(em, mask)
    assert torch.equal(t1, t0) and torch.equal(l1, l0)


# ---- 4. rejected shapes, capture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(8, 65), (513, 17)])
def test_rejected_shapes_launch_nothing(hip, S, C):
    B = 2
    lib = hip.lib()
    em = torch.randn(B, S, C, device=DEV)
    allowed = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    start, end, trans = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, C, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out, dem = torch.full((B,), 7.0, device=DEV), torch.full((B, S, C), 7.0, device=DEV)
    tags = torch.full((B, S), 7, dtype=torch.int32, device=DEV)
    p, st = hip._p, hip._st()
    assert lib.mtvaf_crf_lattice_workspace_bytes(B, S, C) == 0
    assert lib.mtvaf_crf_lattice_fwd(p(em), p(allowed), p(mask), p(start), p(end), p(trans), p(out), None, None, B, S, C, p(ws),
                                     ws.numel(), st) == -1
    assert lib.mtvaf_crf_lattice_bwd(p(out), p(em), p(allowed), p(mask), p(start), p(end), p(trans), p(dem), p(start), p(end),
                                     p(trans), 0, B, S, C, p(ws), ws.numel(), st) == -1
    assert lib.mtvaf_crf_lattice_marginals(p(em), p(allowed), p(mask), p(start), p(end), p(trans), p(dem), None, B, S, C, p(ws),
                                           ws.numel(), st) == -1
    assert lib.mtvaf_crf_lattice_viterbi(p(em), p(allowed), p(mask), p(start), p(end), p(trans), p(tags), p(tags), None, B, S, C,
                                         st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((dem == 7).all()) and bool((tags == 7).all()) and int(ws.sum()) == 0


def test_small_workspace_is_refused(hip):
    ref = X.reference((3, 17, 11, 1), "c")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    ws, wsb = hip.crf_lattice_workspace(3, 17, 11, DEV)
    with pytest.raises(Exception):
        hip.crf_lattice_fwd(em, ref.allowed.to(DEV), mask, start, end, trans, torch.empty(3, device=DEV), None, None, ws, wsb - 4)


def test_graph_capture_replays_the_eager_bits(hip):
    """lattice_fwd -> lattice_bwd -> lattice_viterbi on one stream as a single linear chain, captured, replayed once."""
    ref = X.reference((3, 65, 11, 1), "c")
    em, _, mask, start, end, trans = _dev(*ref.inputs)
    allowed, w = _dev(ref.allowed, ref.w)
    B, S, C = em.shape
    ws, wsb = hip.crf_lattice_workspace(B, S, C, DEV)

    def buffers():
        return dict(pllh=torch.zeros(B, device=DEV), logz_a=torch.zeros(B, device=DEV), logz=torch.zeros(B, device=DEV),
                    dem=torch.zeros(B, S, C, device=DEV), ds=torch.zeros(C, device=DEV), de=torch.zeros(C, device=DEV),
                    dt=torch.zeros(C, C, device=DEV), tags=torch.zeros(B, S, dtype=torch.int32, device=DEV),
                    lens=torch.zeros(B, dtype=torch.int32, device=DEV), score=torch.zeros(B, device=DEV))

    def chain(o):
        hip.crf_lattice_fwd(em, allowed, mask, start, end, trans, o["pllh"], o["logz_a"], o["logz"], ws, wsb)
        hip.crf_lattice_bwd(w, em, allowed, mask, start, end, trans, o["dem"], o["ds"], o["de"], o["dt"], False, ws, wsb)
        hip.crf_lattice_viterbi(em, allowed, mask, start, end, trans, o["tags"], o["lens"], o["score"])

    eager, cap = buffers(), buffers()
    chain(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(cap)
    for v in cap.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    X.check(ref, "pllh", cap["pllh"])


# ---- 5. the model ------------------------------------------------------------------------------------------------------------
LABELS = E.SET_A
LABEL_MAP = {label: i for i, label in enumerate(LABELS, 1)}


def tiny_model(**kw):
    """The tiny configuration of test_crf_entities_gpu.py, without the visual prefix."""
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=False, vao=False, noauxloss=False,
                                 use_probe=False, n_gpu=1, alpha=0.5, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV,
                                 resnet_root=None, use_152=False, **kw)
    args.bert_config = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                                  num_attention_heads=cfg.heads, intermediate_size=cfg.inter,
                                  max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.eps,
                                  hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    with torch.no_grad():  # an untrained head decodes mostly one tag: spread the emissions
        m.fc.weight.mul_(40.0)
    return cfg, m


def test_predict_constrained():
    from mtvaf_amd.metrics import structural_labels
    cfg, m = tiny_model(max_entities=16)
    B, S = 6, 32
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt)
    words = (torch.rand(B, S, generator=torch.Generator().manual_seed(3)) < 0.7).to(DEV)
    m.eval()
    C = len(LABELS) + 1
    # full sets: `predict`, in every returned tensor
    for full in (torch.zeros(B, S, dtype=torch.int64, device=DEV), torch.full((B, S), (1 << C) - 1, dtype=torch.int64, device=DEV)):
        free, same = m.predict(**kw, word_mask=words), m.predict_constrained(**kw, word_mask=words, allowed=full)
        assert set(free) == set(same) and free["types"] == same["types"]
        for k, v in free.items():
            if torch.is_tensor(v):
                assert torch.equal(v, same[k]), k
    # the default structural sets: no structural tag on a word column, nothing but X on a piece column
    res = m.predict_constrained(**kw, word_mask=words)
    tags, n = res["tags"].cpu(), X.lengths_of(mask.cpu())
    structural = {LABEL_MAP.get(name, 0) for name in structural_labels(LABEL_MAP)}
    seen_word = seen_piece = 0
    for b in range(B):
        L_b = int(n[b])
        assert int(tags[b, 0]) == LABEL_MAP["[CLS]"] and (L_b == 1 or int(tags[b, L_b - 1]) == LABEL_MAP["[SEP]"])
        for t in range(1, L_b - 1):
            if bool(words[b, t]):
                assert int(tags[b, t]) not in structural
                seen_word += 1
            else:
                assert int(tags[b, t]) == LABEL_MAP["X"]
                seen_piece += 1
    assert seen_word > 10 and seen_piece > 10


def test_forward_with_allowed_tags():
    from mtvaf_amd import engine
    from mtvaf_amd.constraints import sets_from_labels
    cfg, m = tiny_model(crf_reduction="token_mean")
    B, S = 6, 32
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt)
    C = len(LABELS) + 1

    def step(**extra):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        out = m.train()(**kw, **extra)
        out.loss.backward()
        return float(out.loss), m.fc.weight.grad.detach().double().cpu().clone()

    loss_l, g_l = step(labels=labels)
    loss_a, g_a = step(allowed_tags=sets_from_labels(labels, C))
    # the two losses are the same quantity: both inside the likelihood bound of the rule, scaled as the losses are
    tol_loss = 2 * 2e-5 * max(abs(loss_l), 1.0)
    print(f"forward(allowed_tags) loss {loss_a:.6f} vs {loss_l:.6f}; grad err {float((g_a - g_l).abs().max()):.3e}")
    assert abs(loss_a - loss_l) <= tol_loss
    assert float((g_a - g_l).abs().max()) <= 2 * (1e-4 * float(g_l.abs().max()) + 1e-7)
    assert m(**kw).loss is None


def test_unknown_sentence_moves_nothing():
    """A batch in which one sentence is all-unknown: its emission gradients are exact zeros."""
    from mtvaf_amd.constraints import sets_from_labels
    from mtvaf_amd.modules.crf import CRF
    ref = X.reference((3, 17, 11, 1), "b")
    em, tags, mask, start, end, trans = _dev(*ref.inputs)
    crf = CRF(11, batch_first=True).to(DEV)
    labels = tags.clone()
    labels[0] = -100
    e = em.clone().requires_grad_(True)
    pllh = crf.partial_llh(e, sets_from_labels(labels, 11), mask)
    (-pllh.sum()).backward()
    assert float(pllh[0]) == 0.0 and bool((e.grad[0] == 0).all()) and bool((e.grad[1] != 0).any())
