"""Candidate-span proposal on the MI355X: `mtvaf_span_propose` against the restatement of its rule over the case table and against
the lists recorded from the reference, its input conventions, determinism, graph capture, and `TVNetSAModel.predict` end to end.
Outputs are integers (and the fp32 rounding of an fp64 sum): every comparison is exact."""
import numpy as np
import pytest
import torch

import params as P
import span_propose_cases as C
from test_model_gpu import DEV, hf_config, load, make_args, LABELS
from test_span_propose import golden_cases

pytestmark = pytest.mark.gpu

KEYS = ("span_starts", "span_ends", "label_masks", "span_scores", "count")


def run_kernel(sl, el, wi, wk, n_best, max_len, thr, heur, nms):
    from mtvaf_amd import hip
    ae = torch.from_numpy(np.stack([sl, el], -1)).to(DEV)
    out = hip.span_propose(ae, torch.from_numpy(wi).to(DEV), None if wk is None else torch.from_numpy(wk).to(DEV), n_best=n_best,
                           max_len=max_len, threshold=thr, use_heuristics=heur, nms=nms)
    return dict(zip(KEYS, out))


def assert_same(got, ref, what=""):
    for k in KEYS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, (what, k, g.dtype, g.shape)
        if k == "span_scores":
            g, r = g.view(np.int32), ref[k].view(np.int32)  # bit-equal
        else:
            r = ref[k]
        assert np.array_equal(g, r), (what, k, np.argwhere(g != r)[:4].tolist())


@pytest.mark.parametrize("case", C.TABLE, ids=[c[0] for c in C.TABLE])
def test_kernel_equals_restatement(case):
    name, B, S, n_best, max_len, heur, nms, keyed = case
    sl, el, wi, wk = C.make_inputs(B, S, seed=1000 + 7 * S + B)
    wk = wk if keyed else None
    ref = C.propose(sl, el, wi, wk, n_best, max_len, C.THRESHOLD, heur, nms)
    assert_same(run_kernel(sl, el, wi, wk, n_best, max_len, C.THRESHOLD, heur, nms), ref, name)
    if B >= 3 and S > 3:
        assert ref["count"][1] == 0  # the all-filtered row
    if B == 70 and max_len == 12 and nms == 0:
        assert ref["count"].max() == (n_best + 1) // 2  # some row fills the list


def test_kernel_equals_reference_lists():
    for g in golden_cases():
        got = run_kernel(g["sl"], g["el"], g["wi"], g["wk"], g["n_best"], g["max_len"], g["thr"], g["heur"], g["nms"])
        for k in ("span_starts", "span_ends", "label_masks"):
            assert np.array_equal(got[k].cpu().numpy(), g[k]), (g["c"], k)
        assert np.array_equal(got["count"].cpu().numpy(), g["label_masks"].sum(1))


def test_strided_input_repeat_call_and_model_entry():
    """ld = 2 (the binary_affine output) and ld = 4 (two columns of a wider tensor) against separate contiguous start / end copies
    through TVNetSAModel.propose_spans' three input forms; a second call gives the same bits."""
    from mtvaf_amd import hip
    from mtvaf_amd.models.bert_model import TVNetSAModel
    B, S, n_best = 5, 70, 20
    sl, el, wi, wk = C.make_inputs(B, S, seed=77)
    ref = C.propose(sl, el, wi, wk, n_best, 12, C.THRESHOLD, 1, 0)
    wide = torch.zeros(B, S, 4)
    wide[..., 1], wide[..., 2] = torch.from_numpy(sl), torch.from_numpy(el)
    wide = wide.to(DEV)
    wit, wkt = torch.from_numpy(wi).to(DEV), torch.from_numpy(wk).to(DEV)
    kw = dict(n_best=n_best, max_len=12, threshold=C.THRESHOLD, use_heuristics=True, nms=0)
    view = wide[..., 1:3]
    assert view.stride(1) == 4 and not view.is_contiguous()
    assert_same(dict(zip(KEYS, hip.span_propose(view, wit, wkt, **kw))), ref, "ld=4")
    ae = view.contiguous()
    first = hip.span_propose(ae, wit, wkt, **kw)
    assert_same(dict(zip(KEYS, first)), ref, "ld=2")
    again = hip.span_propose(ae, wit, wkt, **kw)
    assert all(torch.equal(a, b) for a, b in zip(first, again))

    import types
    model = types.SimpleNamespace(args=make_args(n_best_size=n_best, max_answer_length=12, logit_threshold=C.THRESHOLD, use_heuristics=True, use_nms=False))
    model.propose_spans = lambda *a, **k: TVNetSAModel.propose_spans(model, *a, **k)  # the method reads self.args only
    forms = {"columns of one tensor": (ae[..., 0], ae[..., 1]), "contiguous copies": (ae[..., 0].contiguous(), ae[..., 1].contiguous()),
             "[B,S,2]": (ae, None)}
    for what, (a, b) in forms.items():
        assert_same(dict(zip(KEYS, model.propose_spans(a, b, None, token_to_word=wit, word_key=wkt))), ref, what)
    # defaults: token_to_word from the attention mask (every token its own word), positional keys
    mask = torch.from_numpy((wi >= 0).astype(np.int64)).to(DEV)
    pos = np.where(wi >= 0, np.arange(S, dtype=np.int32)[None], -1).astype(np.int32)
    assert_same(dict(zip(KEYS, model.propose_spans(ae, None, mask))), C.propose(sl, el, pos, None, n_best, 12, C.THRESHOLD, 1, 0),
                "mask default")
    model.args.use_nms = True
    assert_same(dict(zip(KEYS, model.propose_spans(ae, None, None, token_to_word=wit, word_key=wkt))),
                C.propose(sl, el, wi, wk, n_best, 12, C.THRESHOLD, 1, 1), "use_nms f1")
    model.args.filter_type = "em"
    assert_same(dict(zip(KEYS, model.propose_spans(ae, None, None, token_to_word=wit, word_key=wkt))), ref, "use_nms em")


def test_graph_capture_replays_on_new_logits():
    """One capture of the call in a single-stream graph, replayed after the logits changed in place: no host sync in the call."""
    from mtvaf_amd import hip
    B, S, n_best = 3, 64, 20
    sl, el, wi, wk = C.make_inputs(B, S, seed=5)
    sl2, el2, _, _ = C.make_inputs(B, S, seed=6)
    ae = torch.from_numpy(np.stack([sl, el], -1)).to(DEV)
    wit, wkt = torch.from_numpy(wi).to(DEV), torch.from_numpy(wk).to(DEV)
    kw = dict(n_best=n_best, max_len=12, threshold=C.THRESHOLD, use_heuristics=True, nms=1)
    hip.span_propose(ae, wit, wkt, **kw)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.span_propose(ae, wit, wkt, **kw)
    graph.replay()
    assert_same(dict(zip(KEYS, out)), C.propose(sl, el, wi, wk, n_best, 12, C.THRESHOLD, 1, 1), "replay 1")
    ae.copy_(torch.from_numpy(np.stack([sl2, el2], -1)))
    graph.replay()
    ref2 = C.propose(sl2, el2, wi, wk, n_best, 12, C.THRESHOLD, 1, 1)
    assert_same(dict(zip(KEYS, out)), ref2, "replay 2")
    assert not np.array_equal(ref2["span_starts"], C.propose(sl, el, wi, wk, n_best, 12, C.THRESHOLD, 1, 1)["span_starts"])


def test_predict_end_to_end():
    """TVNetSAModel.predict on the tiny config of the tvnet1_tiny_B3S16 fixture, eval mode: its spans are the rule applied to the
    logits it returns, its polarity logits are `classification` on those spans bit for bit (same kernels, same inputs)."""
    from mtvaf_amd.models.bert_model import TVNetSAModel
    fx = load("tvnet1_tiny_B3S16")
    cfg = P.TINY_BERT_L8
    seed, B, S = int(fx["seed"]), int(fx["B"]), int(fx["S"])
    lengths = [int(x) for x in fx["lengths"]]
    sd = {**{"bert." + k: v for k, v in P.encoder_params(cfg, seed).items()}, **P.span_head_params(cfg, seed + 3)}
    args = make_args(use_prefix=False, gcn_layer_number=0, num_layers=0)
    args.bert_config = hf_config(cfg)
    m = TVNetSAModel(LABELS, None, args)
    assert not m.load_state_dict(sd, strict=False)[1]
    m = m.to(DEV).eval()
    ids, mask, tt, _ = (t.to(DEV) for t in P.text_batch(cfg, seed + 1, B, S, lengths))
    pos = np.where(mask.cpu().numpy() != 0, np.arange(S, dtype=np.int32)[None], -1).astype(np.int32)

    def check(thr, n_best=20):
        out = m.predict(ids, mask, tt)
        sl, el = out["start_logits"].cpu().numpy(), out["end_logits"].cpu().numpy()
        ref = C.propose(sl, el, pos, None, n_best, 12, thr, 1, 0)
        for k in ("span_starts", "span_ends", "label_masks", "span_scores"):
            g = out[k].cpu().numpy()
            assert g.dtype == ref[k].dtype and np.array_equal(g.view(np.int32) if k == "span_scores" else g,
                                                              ref[k].view(np.int32) if k == "span_scores" else ref[k]), k
        with torch.no_grad():
            _, seq = m._extract(mask, ids, None, tt)
            logits, _ = m.classification(out["span_starts"], out["span_ends"], seq, mask)
        assert tuple(out["logits"].shape) == (B, n_best, 4) and torch.equal(out["logits"], logits)
        assert not out["logits"].requires_grad
        return out, float((sl.max(1) + el.max(1)).min())

    out, top = check(8.0)  # the reference's defaults (read through _arg: args sets none of them)
    m.args.logit_threshold = top - 100.0
    out, _ = check(top - 100.0)
    assert int(out["label_masks"].sum()) >= B and bool((out["label_masks"].sum(1) > 0).all())
