"""Word-level tagging head on the MI355X: mtvaf_word_index / mtvaf_word_pool_fwd / mtvaf_word_pool_bwd
against the restatement and the derived bounds of wordpool_cases.py, and `TVNetSAModel2` with args.word_pooling against a hand
composition -- eager float64 pooling of the model's own last_hidden_state, then the same fc and CRF -- on the tiny models of
test_model_gpu (dropout 0, eval mode)."""
import functools

import numpy as np
import pytest
import torch

import entity_cases as E
import params as P
import wordpool_cases as WC
from test_model_gpu import LABELS, close, hf_config, make_args
from test_ops_gpu import DEV, hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _ref(i):
    """Inputs and the index restatement of case i, computed once and never written to."""
    mask, t2w, W = WC.make_index_inputs(WC.CASES[i])
    return mask, t2w, W, WC.index_reference(mask, t2w, W)


@functools.lru_cache(maxsize=None)
def _pool_ref(i, mode):
    mask, t2w, W, ref = _ref(i)
    x, dy = WC.make_x(WC.CASES[i]), WC.make_x(WC.CASES[i], seed=1, width=W)
    return x, dy, WC.pool_reference(x, ref, mode), WC.pool_bwd_reference(dy, ref, mode)


def _dev(ref):
    return {k: v.to(DEV) for k, v in ref.items()}


def _prefilled(mask, W):
    B, S = mask.shape
    i32 = lambda *shape: torch.full(shape, WC.SENTINEL, dtype=torch.int32, device=DEV)
    return dict(col_start=i32(B, W), col_len=i32(B, W), col_of_token=i32(B, S), word_id=i32(B, W), n_cols=i32(B),
                word_mask=torch.full((B, W), 77, dtype=torch.uint8, device=DEV))


def _misaligned(t):
    """The same values in a view that starts 4 bytes past a 16-byte boundary: the kernels take their scalar path."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---- 1. the index --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(WC.CASES)), ids=WC.IDS)
def test_index_equals_the_restatement_and_writes_every_element(hip, i):
    mask, t2w, W, ref = _ref(i)
    out = _prefilled(mask, W)
    got = hip.word_index(mask.to(DEV), t2w.to(DEV), W, out=out)
    torch.cuda.synchronize()
    for k, v in ref.items():
        assert got[k] is out[k] and got[k].dtype == v.dtype
        assert torch.equal(got[k].cpu(), v), k
    again = hip.word_index(mask.to(DEV), t2w.to(DEV), W)
    assert all(torch.equal(again[k], got[k]) for k in ref), "same inputs, same bits"
    # masks of other dtypes read as non-zero = live
    assert all(torch.equal(hip.word_index(mask.to(DEV).long(), t2w.to(DEV), W)[k], got[k]) for k in ref)


def test_index_never_reads_the_map_behind_the_mask(hip):
    for i in range(len(WC.CASES)):
        mask, t2w, W, ref = _ref(i)
        gen = torch.Generator().manual_seed(9)
        junk = torch.where(mask == 0, torch.randint(-(2 ** 31), 2 ** 31 - 1, t2w.shape, generator=gen).to(torch.int32), t2w)
        got = hip.word_index(mask.to(DEV), junk.to(DEV), W)
        assert all(torch.equal(got[k].cpu(), ref[k]) for k in ref), WC.IDS[i]


# ---- 2. forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WC.MODES)
@pytest.mark.parametrize("i", range(len(WC.CASES)), ids=WC.IDS)
def test_forward_matches_the_restatement(hip, i, mode):
    mask, t2w, W, ref = _ref(i)
    x, _, (y64, tol), _ = _pool_ref(i, mode)
    idx = _dev(ref)
    out = torch.full((x.shape[0], W, x.shape[2]), NAN, device=DEV)
    y = hip.word_pool_fwd(x.to(DEV), idx["col_start"], idx["col_len"], mode, out=out)
    torch.cuda.synchronize()
    assert y is out and not bool(torch.isnan(y).any()), "every element is written"
    if mode == "mean":
        ex = WC.excess(y, y64, tol)
        print(f"{WC.IDS[i]} mean forward: excess {ex:.3f} of the derived bound")
        assert ex <= 1.0, ex
        one = (ref["col_len"] == 1)
        assert torch.equal(y.cpu()[one], y64.float()[one]), "a word of one piece is that piece"
    else:
        assert torch.equal(y.cpu(), y64.float())
    assert not bool(y.cpu()[ref["word_mask"] == 0].any()), "dead columns are exact zeros"
    y2 = hip.word_pool_fwd(x.to(DEV), idx["col_start"], idx["col_len"], mode)
    assert torch.equal(y, y2), "same inputs, same bits"
    # the scalar path (a 4-byte-misaligned view of x, and of the output) gives the same values
    y3 = hip.word_pool_fwd(_misaligned(x.to(DEV)), idx["col_start"], idx["col_len"], mode, out=_misaligned(torch.full_like(y, NAN)))
    assert torch.equal(y, y3)


# ---- 3. backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WC.MODES)
@pytest.mark.parametrize("i", range(len(WC.CASES)), ids=WC.IDS)
def test_backward_matches_the_restatement(hip, i, mode):
    mask, t2w, W, ref = _ref(i)
    x, dy, _, (dx64, tol) = _pool_ref(i, mode)
    idx = _dev(ref)
    out = torch.full(tuple(x.shape), NAN, device=DEV)
    dx = hip.word_pool_bwd(dy.to(DEV), idx["col_start"], idx["col_len"], idx["col_of_token"], mode, out=out)
    torch.cuda.synchronize()
    assert dx is out and not bool(torch.isnan(dx).any()), "every element is written"
    if mode == "mean":
        ex = WC.excess(dx, dx64, tol)
        print(f"{WC.IDS[i]} mean backward: excess {ex:.3f} of one rounding")
        assert ex <= 1.0, ex
    else:
        assert torch.equal(dx.cpu(), dx64.float())
    assert not bool(dx.cpu()[dx64 == 0].any()), "masked tokens, dropped columns and unselected pieces are exact zeros"
    dx2 = hip.word_pool_bwd(dy.to(DEV), idx["col_start"], idx["col_len"], idx["col_of_token"], mode)
    assert torch.equal(dx, dx2), "same inputs, same bits"
    dx3 = hip.word_pool_bwd(_misaligned(dy.to(DEV)), idx["col_start"], idx["col_len"], idx["col_of_token"], mode,
                            out=_misaligned(torch.full_like(dx, NAN)))
    assert torch.equal(dx, dx3)


# ---- 4. what the kernels must not read -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WC.MODES)
def test_poison_at_masked_tokens_and_dead_columns_changes_no_bit(hip, mode):
    for i in range(len(WC.CASES)):
        mask, t2w, W, ref = _ref(i)
        x, dy, _, _ = _pool_ref(i, mode)
        idx = _dev(ref)
        y0 = hip.word_pool_fwd(x.to(DEV), idx["col_start"], idx["col_len"], mode)
        dx0 = hip.word_pool_bwd(dy.to(DEV), idx["col_start"], idx["col_len"], idx["col_of_token"], mode)
        for bad in (NAN, float("inf")):
            xp, dyp = x.clone(), dy.clone()
            xp[mask == 0] = bad
            dyp[ref["word_mask"] == 0] = bad
            assert torch.equal(hip.word_pool_fwd(xp.to(DEV), idx["col_start"], idx["col_len"], mode), y0), WC.IDS[i]
            assert torch.equal(hip.word_pool_bwd(dyp.to(DEV), idx["col_start"], idx["col_len"], idx["col_of_token"], mode), dx0), WC.IDS[i]


def test_an_index_that_points_outside_is_dead_and_bad_arguments_stop_at_the_host(hip):
    x = torch.ones(1, 4, 8, device=DEV)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    start, length = i32([0, 3, -1, 2]), i32([1, 2, 1, 5])  # column 1 ends past the sentence, 2 starts before it, 3 is too long
    y = hip.word_pool_fwd(x, start, length, "mean")
    assert torch.equal(y[0, 0], x[0, 0]) and not bool(y[0, 1:].any())
    cols = i32([0, 7, -3, 0])  # a column beyond W, a negative one, a token (3) outside the column it names (0: token 0 alone)
    dx = hip.word_pool_bwd(torch.ones(1, 4, 8, device=DEV), start, length, cols, "mean")
    assert torch.equal(dx[0, 0], x[0, 0]) and not bool(dx[0, 1:].any())
    with pytest.raises(ValueError):
        hip.word_pool_fwd(x, start, length, "max")
    with pytest.raises(ValueError):
        hip.word_pool_fwd(x, start.long(), length, "first")
    with pytest.raises(ValueError):
        hip.word_index(torch.ones(1, 4, dtype=torch.uint8, device=DEV), torch.zeros(1, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.word_index(torch.ones(1, 513, dtype=torch.uint8, device=DEV), torch.zeros(1, 513, dtype=torch.int32, device=DEV))


def test_autograd_node_saves_the_index_only(hip):
    from mtvaf_amd.words import WordPooling, build_word_index
    mask, t2w, W, ref = _ref(5)
    x, dy, (y64, tol), (dx64, dtol) = _pool_ref(5, "mean")
    index = build_word_index(mask.to(DEV), t2w, W)  # (the map may live on the host, in any integer dtype)
    xg = x.to(DEV).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = WordPooling("mean")(xg, index)
    assert not saved, "nothing is saved through autograd: the backward needs the index alone"
    y.backward(dy.to(DEV))
    assert WC.excess(y, y64, tol) <= 1.0 and WC.excess(xg.grad, dx64, dtol) <= 1.0


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
CFG = P.EncCfg(vocab_size=600, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
LABEL_MAP = {label: i for i, label in enumerate(LABELS, 1)}


def _tagger(**kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    args = make_args(alpha=0.0, use_prefix=False, **kw)
    args.bert_config = hf_config(CFG, dropout=0.0)
    torch.manual_seed(11)
    return TVNetSAModel2(LABELS, None, args).to(DEV).eval()


def _batch(B=16, S=64, seed=5, identity=False):
    """-> forward()'s keyword tensors on the device and the word map: [CLS], words of 1 - 3 pieces, [SEP] per sentence."""
    ids, mask, tt, labels = P.text_batch(CFG, seed, B, S, lo_id=5)
    labels[:, 0] = LABEL_MAP["[CLS]"]
    gen = torch.Generator().manual_seed(seed)
    lengths = mask.sum(1).tolist()
    if identity:
        pos = torch.arange(S, dtype=torch.int32)[None, :].expand(B, S)
        t2w = torch.where(mask != 0, pos, torch.full_like(pos, -1))
    else:
        t2w = torch.tensor([WC.sentence(S, n, WC._random_pieces(gen, n, hi=3)) for n in lengths], dtype=torch.int32)
    kw = dict(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), token_type_ids=tt.to(DEV), labels=labels.to(DEV))
    return kw, t2w, mask


def _grads(m):
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


def _hand(m, kw, t2w, mask, mode):
    """Eager float64 pooling of the model's own last_hidden_state, then the same fc and CRF -> loss, emissions, index, labels."""
    from mtvaf_amd import engine
    from mtvaf_amd.words import WordIndex, word_labels
    ref = WC.index_reference(mask.to(torch.uint8), t2w, mask.shape[1])
    idx = _dev(ref)
    bo = m.bert(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], token_type_ids=kw["token_type_ids"],
                output_hidden_states=True, return_dict=True)
    pooled = WC.eager_pool(bo["last_hidden_state"].double(), idx, mode).float()
    em = engine.LinearFunction.apply(pooled, m.fc.weight, m.fc.bias, False)
    wl = word_labels(kw["labels"], WordIndex(**idx))
    loss = m.crf.nll_mean(em, wl, mask=idx["word_mask"])
    return loss, em, idx, wl


def test_identity_map_first_piece_is_the_plain_forward():
    m = _tagger(word_pooling="first")
    kw, t2w, mask = _batch(identity=True)
    out = m(**kw, token_to_word=t2w.to(DEV))
    out.loss.backward()
    tags, g1 = list(out.logits), _grads(m)
    assert torch.equal(m.last_word_index.word_mask.cpu(), mask.to(torch.uint8))
    m.args.word_pooling = None
    plain = m(**kw)
    plain.loss.backward()
    g0 = _grads(m)
    assert torch.equal(out.loss, plain.loss) and tags == list(plain.logits)
    assert set(g0) == set(g1)
    for n in g0:
        close(g1[n], g0[n], name=n)


@pytest.mark.parametrize("mode", WC.MODES)
def test_general_map_matches_the_hand_composition(mode, pad_mode):
    m = _tagger(word_pooling=mode)
    kw, t2w, mask = _batch()
    out = m(**kw, token_to_word=t2w.to(DEV))
    out.loss.backward()
    tags, g1 = list(out.logits), _grads(m)
    loss, em, idx, wl = _hand(m, kw, t2w, mask, mode)
    loss.backward()
    g0 = _grads(m)
    for k, v in idx.items():
        assert torch.equal(getattr(m.last_word_index, k), v), k
    close(out.loss, loss, name="loss")
    assert tags == m.crf.decode(em.detach(), idx["word_mask"])
    assert [len(t) for t in tags] == idx["n_cols"].tolist()
    assert set(g0) == set(g1) and "bert.encoder.layer.0.attention.self.query.weight" in g1
    for n in g0:
        close(g1[n], g0[n], name=n)


def test_padding_free_and_padded_runs_agree_on_the_word_axis():
    """The criterion of tests/test_unpad_gpu.py: the loss within 2e-6 relative, the tags equal."""
    from mtvaf_amd import engine
    m = _tagger(word_pooling="mean")
    kw, t2w, mask = _batch()
    res = []
    for unpad in (False, True):
        with engine.padding_free(unpad):
            out = m(**kw, token_to_word=t2w.to(DEV))
            res.append((float(out.loss.detach()), list(out.logits), engine.LAST_PACK is not None))
    (l0, t0, p0), (l1, t1, p1) = res
    assert not p0 and p1, "the second run did not pack"
    assert abs(l0 - l1) <= 2e-6 * abs(l0) and t0 == t1


def test_predict_returns_the_entities_of_the_hand_composed_emissions_in_word_columns():
    m = _tagger(word_pooling="mean")
    kw, t2w, mask = _batch(B=8, S=32)
    args3 = (kw["input_ids"], kw["attention_mask"], kw["token_type_ids"])
    got = m.predict(*args3, token_to_word=t2w.to(DEV))
    with torch.no_grad():
        _, em, idx, _ = _hand(m, kw, t2w, mask, "mean")
        wm = idx["word_mask"]
        tags, _ = m.crf.decode_packed(em, wm)
        t = m._entity_tables(em.device)
        keep = torch.zeros_like(wm, dtype=torch.bool)
        keep[:, 1:] = torch.cumprod(wm[:, 1:], dim=1).bool()
        keep &= ~t["structural"][tags.clamp(0, t["C"] - 1).long()]
        want = m.crf.entities(em, wm, t, tags=tags, keep=keep, max_entities=32)
    torch.cuda.synchronize()
    assert tuple(got["tags"].shape) == tuple(wm.shape)
    for k in ("tags", "lengths", "entities", "count"):
        assert torch.equal(got[k], want[k]), k
    close(got["log_confidence"], want["log_confidence"], name="log_confidence")
    assert int(got["count"].sum()) > 0 and int(got["entities"][..., :2].max()) < int(idx["n_cols"].max())
    # the other entry points take the map the same way, and refuse word_mask beside it
    assert torch.equal(m.predict_nbest(*args3, token_to_word=t2w.to(DEV), nbest=2)["tags"][:, 0], got["tags"])
    con = m.predict_constrained(*args3, token_to_word=t2w.to(DEV))
    assert tuple(con["tags"].shape) == tuple(wm.shape)
    post = m.predict_posteriors(*args3, token_to_word=t2w.to(DEV))
    assert torch.equal(post["decoded"]["tags"], con["tags"]) and post["keep"].shape == wm.shape
    with pytest.raises(ValueError, match="word_mask"):
        m.predict(*args3, word_mask=kw["attention_mask"], token_to_word=t2w.to(DEV))
    with pytest.raises(ValueError, match="token_to_word"):
        m.predict(*args3)
    with pytest.raises(ValueError, match="token_to_word"):
        m(**kw)


def test_entity_scorer_counts_word_columns():
    from mtvaf_amd.words import word_labels
    m = _tagger(word_pooling="first", score_entities=True)
    kw, t2w, mask = _batch(B=8, S=32)
    out = m(**kw, token_to_word=t2w.to(DEV))
    torch.cuda.synchronize()
    index = m.last_word_index
    gold = word_labels(kw["labels"], index).cpu().numpy()
    pred = out.logits.device_tags.cpu().numpy()
    sc = m.entity_scorer
    want = E.counter(sc.types, E.restate(LABEL_MAP, "seqeval", gold, pred, index.word_mask.cpu().numpy()))
    assert sc.counts.cpu().numpy().tolist() == want.tolist() and want[-1] > 0


def test_forward_without_the_new_argument_is_unchanged_by_word_axis_calls_in_between():
    m = _tagger()
    kw, t2w, mask = _batch(B=8, S=32)

    def plain():
        out = m(**kw)
        out.loss.backward()
        return out.loss.detach().clone(), list(out.logits), _grads(m)
    l0, t0, g0 = plain()
    assert m.last_word_index is None
    m.args.word_pooling = "mean"
    m(**kw, token_to_word=t2w.to(DEV)).loss.backward()
    _grads(m)
    m.args.word_pooling = None
    l1, t1, g1 = plain()
    assert torch.equal(l0, l1) and t0 == t1 and set(g0) == set(g1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    # without args.word_pooling a map is not read: the piece-level head runs
    l2 = m(**kw, token_to_word=t2w.to(DEV)).loss
    assert torch.equal(l0, l2.detach())


def test_graph_replay_with_the_map_in_the_static_batch_equals_the_eager_step():
    from mtvaf_amd import engine
    from mtvaf_amd.graph import GraphedTrainStep
    m = _tagger(word_pooling="mean")
    kw, t2w, mask = _batch(B=4, S=64)
    kw = dict(kw, token_to_word=t2w.to(DEV))

    def eager():  # (returns plain values: a live autograd graph of an earlier step must not reach the capture)
        m.zero_grad(set_to_none=True)
        out = m(**kw)
        out.loss.backward()
        torch.cuda.synchronize()
        return float(out.loss), list(out.logits), m.fc.weight.grad.clone()

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
            assert torch.equal(m.fc.weight.grad, egrad)
        finally:
            g.close()
    finally:
        engine.UNPAD = was
