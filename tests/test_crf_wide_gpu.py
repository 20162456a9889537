"""Wide-tag CRF kernels (csrc/crf_wide.hip, 17 <= C <= 64) through the C ABI, the CRF module and TVNetSAModel2 on the
MI355X: loss and gradients against the float64 oracle with the bounds of the 16-tag kernels' tests, Viterbi paths under
the near-tie rule of crf_wide_cases.viterbi_near_ties, brute-force known answers, error codes, graph capture."""
import types

import pytest
import torch
from transformers import BertConfig

import crf_wide_cases as W
import params as P
from oracle import mtvaf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


def close(got, ref, rtol, atol=None, name=""):
    got = torch.as_tensor(got).detach().float().cpu()
    ref = torch.as_tensor(ref).detach().float().cpu()
    if atol is None:
        atol = rtol * float(ref.abs().max()) + 1e-7
    err = (got - ref).abs()
    print(f"{name}: max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})")
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{name}: max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), " \
                                f"{int(bad.sum())}/{bad.numel()} bad"


def _decode(hip, em, mask, start, end, trans):
    B, S, _ = em.shape
    g = lambda t: t.to(DEV)
    tg, ln = torch.empty(B, S, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    hip.crf_viterbi(g(em), g(mask), g(start), g(end), g(trans), tg, ln)
    tg, ln = tg.cpu(), ln.cpu()
    assert all(int((row[int(n):] != -1).sum()) == 0 for row, n in zip(tg, ln))
    assert ln.tolist() == mask.long().sum(1).tolist()
    return [[int(t) for t in row[: int(n)]] for row, n in zip(tg, ln)]


@pytest.mark.parametrize("B,S,C,scale", W.FIXED)
def test_crf_wide(hip, B, S, C, scale):
    """scale > 1: emissions and transitions spread over tens of nats; scale < 0: masks with holes (pytorch-crf carries
    the score over a masked step).  grad_out = 1.7 accumulated onto ones.  C = 33 / 64 use lanes >= 32, C = 17, 21
    and 48 leave the last 16-lane row partly empty."""
    em, tags, mask, start, end, trans = W.fixed_case(B, S, C, scale)
    g = lambda t: t.to(DEV)
    emd, sd_, ed, td = (t.double().requires_grad_(True) for t in (em, start, end, trans))
    ref = -O.crf_log_likelihood(emd, tags, mask, sd_, ed, td, "mean")
    (ref * 1.7).backward()
    ws, wsb = hip.crf_workspace(B, S, C, DEV)
    loss = torch.empty(1, device=DEV)
    args = (g(em), g(tags), g(mask), g(start), g(end), g(trans))
    hip.crf_nll_fwd(*args, loss, ws, wsb)
    close(loss, ref.reshape(1), rtol=1e-5, name="crf loss")
    dem = torch.empty(B, S, C, device=DEV)
    ds, de, dt = torch.ones(C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, C, device=DEV)
    gout = torch.tensor([1.7], device=DEV)
    hip.crf_nll_bwd(gout, *args, dem, ds, de, dt, True, ws, wsb)
    close(dem, emd.grad, rtol=1e-4, atol=1e-6, name="crf dem")
    close(ds, sd_.grad + 1, rtol=1e-4, name="crf dstart")
    close(de, ed.grad + 1, rtol=1e-4, name="crf dend")
    tgrad = td.grad if td.grad is not None else torch.zeros_like(td)  # S == 1: no transition is used
    close(dt, tgrad + 1, rtol=1e-4, name="crf dtrans")
    near, bad = W.viterbi_near_ties(_decode(hip, em, mask, start, end, trans), em, mask, start, end, trans)
    assert not bad and near <= W.viterbi_cap(B), (near, bad)


def test_crf_wide_random_shapes(hip):
    """Thirty random draws, 17 <= C <= 64, 1 <= S <= 512, holes in every third draw: S crosses the 16-step operand chunks
    and the 4-step back-pointer words at arbitrary offsets."""
    g = lambda t: t.to(DEV)
    near_total, n = 0, 0
    for tag, (em, tags, mask, start, end, trans) in W.random_draws():
        B, S, C = em.shape
        emd, sd_, ed, td = (t.double().requires_grad_(True) for t in (em, start, end, trans))
        ref = -O.crf_log_likelihood(emd, tags, mask, sd_, ed, td, "mean")
        ref.backward()
        ws, wsb = hip.crf_workspace(B, S, C, DEV)
        loss = torch.empty(1, device=DEV)
        args = (g(em), g(tags), g(mask), g(start), g(end), g(trans))
        hip.crf_nll_fwd(*args, loss, ws, wsb)
        close(loss, ref.reshape(1), rtol=2e-5, name="crf loss " + tag)
        dem = torch.empty(B, S, C, device=DEV)
        ds, de, dt = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, C, device=DEV)
        hip.crf_nll_bwd(None, *args, dem, ds, de, dt, False, ws, wsb)
        close(dem, emd.grad, rtol=1e-4, atol=2e-6, name="crf dem " + tag)
        close(ds, sd_.grad, rtol=1e-4, atol=2e-6, name="crf dstart " + tag)
        close(de, ed.grad, rtol=1e-4, atol=2e-6, name="crf dend " + tag)
        close(dt, td.grad if td.grad is not None else torch.zeros_like(td), rtol=1e-4, atol=2e-6, name="crf dtrans " + tag)
        near, bad = W.viterbi_near_ties(_decode(hip, em, mask, start, end, trans), em, mask, start, end, trans)
        assert not bad, (tag, bad)
        near_total += near
        n += B
    assert near_total <= W.viterbi_cap(n), (near_total, n)


@pytest.mark.parametrize("B,S,C,seed,lengths", W.BRUTE)
def test_crf_wide_bruteforce_known_answer(hip, B, S, C, seed, lengths):
    em, tags, mask, start, end, trans = W.crf_inputs(B, S, C, seed, lengths=lengths)
    logZ, best = O.crf_bruteforce(em, mask, start, end, trans)
    assert _decode(hip, em, mask, start, end, trans) == best
    g = lambda t: t.to(DEV)
    ws, wsb = hip.crf_workspace(B, S, C, DEV)
    loss = torch.empty(1, device=DEV)
    hip.crf_nll_fwd(g(em), g(tags), g(mask), g(start), g(end), g(trans), loss, ws, wsb)
    sc = O.crf_sequence_score(em, tags, mask, start, end, trans)
    want = -float((sc.double() - torch.tensor(logZ)).mean())
    assert abs(float(loss) - want) < 1e-4 * max(1, abs(want))


@pytest.mark.parametrize("S,C", [(8, 65), (513, 17), (600, 64)])
def test_crf_wide_unsupported_shapes_are_errors(hip, S, C):
    """C > 64, or S > 512 on the wide path: every entry point returns MTVAF_ERR_SHAPE (hip.py raises) and writes nothing."""
    B = 2
    lib = hip.lib()
    assert lib.mtvaf_crf_workspace_bytes(B, S, C) == 0
    em = torch.randn(B, S, C, device=DEV)
    tags = torch.zeros(B, S, dtype=torch.long, device=DEV)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    start, end, trans = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, C, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    with pytest.raises(Exception):
        hip.crf_nll_fwd(em, tags, mask, start, end, trans, loss, ws, ws.numel())
    dem = torch.full((B, S, C), 7.0, device=DEV)
    ds, de, dt = torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV), torch.full((C, C), 7.0, device=DEV)
    with pytest.raises(Exception):
        hip.crf_nll_bwd(None, em, tags, mask, start, end, trans, dem, ds, de, dt, False, ws, ws.numel())
    tg = torch.full((B, S), 7, dtype=torch.int32, device=DEV)
    ln = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    with pytest.raises(Exception):
        hip.crf_viterbi(em, mask, start, end, trans, tg, ln)
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((dem == 7).all()) and bool((dt == 7).all()) and bool((tg == 7).all())
    assert bool((ln == 7).all()) and int(ws.sum()) == 0


def test_crf_wide_module_nll_mean_sum_and_deferred_decode():
    from mtvaf_amd.modules.crf import CRF
    torch.manual_seed(3)
    C = 21
    crf = CRF(C, batch_first=True).to(DEV)
    em = torch.randn(6, 40, C, device=DEV, requires_grad=True)
    tags = torch.randint(0, C, (6, 40), device=DEV)
    mask = (torch.arange(40, device=DEV)[None] < torch.tensor([40, 33, 1, 17, 40, 8], device=DEV)[:, None]).to(torch.uint8)
    a = -1 * crf(em, tags, mask=mask, reduction="mean")
    ga = torch.autograd.grad(a, [em, crf.transitions, crf.start_transitions, crf.end_transitions])
    b = crf.nll_mean(em, tags, mask=mask)
    gb = torch.autograd.grad(b, [em, crf.transitions, crf.start_transitions, crf.end_transitions])
    assert torch.equal(a, b)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    s = crf(em, tags, mask=mask, reduction="sum")
    assert torch.equal(s, -b * 6)
    eager = crf.decode(em.detach(), mask)
    deferred = crf.decode_deferred(em.detach(), mask)
    assert deferred == eager and [len(t) for t in eager] == mask.sum(1).tolist()


LABELS20 = ["O", "B-PER", "I-PER", "E-PER", "S-PER", "B-LOC", "I-LOC", "E-LOC", "S-LOC", "B-ORG", "I-ORG", "E-ORG",
            "S-ORG", "B-MISC", "I-MISC", "E-MISC", "S-MISC", "X", "[CLS]", "[SEP]"]


def _hf_config(cfg, dropout=0.0):
    return BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                      num_attention_heads=cfg.heads, intermediate_size=cfg.inter, max_position_embeddings=cfg.max_pos,
                      type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.eps, hidden_dropout_prob=dropout,
                      attention_probs_dropout_prob=dropout, hidden_act="gelu", pad_token_id=0)


def _args(**kw):
    base = dict(bert_name="bert-base-uncased", use_prefix=False, vao=False, noauxloss=True, use_probe=False, n_gpu=1,
                alpha=0.0, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV, resnet_root=None, use_152=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _tvnet2(cfg, sde, sdh):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = _args()
    args.bert_config = _hf_config(cfg)
    m = TVNetSAModel2(LABELS20, None, args)
    sd = {**{"bert." + k: v for k, v in sde.items()}, **sdh}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    return m.to(DEV)


def test_tvnet2_21_tags_full_size_step_vs_oracle(f32_arith, pad_mode):
    """BASELINE config-2 shape (S=128, P=36) at B=4 with a 20-label list (C = 21) against the CPU oracle, with the bounds
    of test_model_gpu's full-size step: emissions / loss 1e-3, fc and transition gradients 3e-3."""
    cfg = P.EncCfg(vocab_size=30522, hidden=768, heads=12, inter=3072, layers=12, max_pos=512, num_labels=21)
    B, S, Pn = 4, 128, 36
    sde, sdh = P.encoder_params(cfg, 7, std=0.03), P.head_params(cfg, 8)
    m = _tvnet2(cfg, sde, sdh)
    m.eval()
    assert m.crf.num_tags == 21
    ids, mask, tt, labels = P.text_batch(cfg, 9, B, S, lo_id=1000)
    labels[:, 0] = 19
    pkv = P.prefix_kv(10, cfg.layers, B, cfg.heads, Pn, std=0.5)
    sd = {**{"bert." + k: v for k, v in sde.items()}, **{k: v.clone().requires_grad_(True) for k, v in sdh.items()}}
    oloss, oem, otags, ohs = O.tvnet2_forward(sd, ids, mask, tt, labels, pkv, cfg.layers, cfg.heads, cfg.eps)
    oloss.backward()
    full = torch.cat([torch.ones(B, Pn, dtype=mask.dtype), mask], 1).to(DEV)
    gp = [(k.to(DEV), v.to(DEV)) for k, v in pkv]
    bo = m.bert(input_ids=ids.to(DEV), attention_mask=full, token_type_ids=tt.to(DEV), past_key_values=gp)
    from mtvaf_amd import engine
    em = engine.LinearFunction.apply(bo["last_hidden_state"], m.fc.weight, m.fc.bias, False)
    valid = mask.bool().to(DEV)
    close(em[valid], oem[valid.cpu()], rtol=1e-3, name="emissions")
    mask_u8 = mask.to(DEV).to(torch.uint8)
    got = m.crf.decode(em, mask_u8)
    emc = em.detach().cpu()
    start, end, trans = (t.detach().cpu() for t in (m.crf.start_transitions, m.crf.end_transitions, m.crf.transitions))
    near, bad = W.viterbi_near_ties(got, emc, mask.to(torch.uint8), start, end, trans)
    assert not bad and near <= W.viterbi_cap(B), (near, bad)
    loss = -m.crf(em, labels.to(DEV), mask=mask_u8, reduction="mean")
    assert abs(float(loss) - float(oloss)) <= 1e-3 * abs(float(oloss))
    loss.backward()
    close(m.fc.weight.grad, sd["fc.weight"].grad, rtol=3e-3, name="g_fc_w")
    close(m.crf.transitions.grad, sd["crf.transitions"].grad, rtol=3e-3, name="g_trans")


def test_tvnet2_21_tags_graph_replay_equals_eager():
    """One GraphedTrainStep replay at C = 21 gives the eager step's loss and decoded tags bit for bit."""
    from mtvaf_amd import engine
    from mtvaf_amd.graph import GraphedTrainStep
    cfg = P.EncCfg(vocab_size=300, hidden=128, heads=2, inter=256, layers=2, max_pos=64, num_labels=21)
    m = _tvnet2(cfg, P.encoder_params(cfg, 1), P.head_params(cfg, 2))
    m.eval()
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 3, 4, 64, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
    def eager():  # (returns plain values: a live autograd graph of an earlier step must not reach the capture)
        m.zero_grad(set_to_none=True)
        out = m(**kw)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss), list(out.logits), m.crf.transitions.grad.clone()

    was = engine.UNPAD
    engine.UNPAD = False
    try:
        eloss, etags, egrad = eager()
        g = GraphedTrainStep(m, kw)
        try:
            m.zero_grad(set_to_none=True)
            out = g(**kw)
            torch.cuda.synchronize()
            assert float(out.loss) == eloss
            assert list(out.logits) == etags
            assert torch.equal(m.crf.transitions.grad, egrad)
        finally:
            g.close()
    finally:
        engine.UNPAD = was
