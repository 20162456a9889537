"""Tagger inference on the MI355X: `mtvaf_crf_entities` / `CRF.entities` / `TVNetSAModel2.predict` against the references of
tests/crf_entities_cases.py.  Entities and counts are compared exactly with the sequential restatement of the chunk rule; the
log confidence with the float64 constrained partition function under the likelihood rule of tests/crf_llh_cases.py,
    |got - ref64| <= max(2e-5 * max|logZ64|, 4 * max|ref32 - ref64|),
printed as err / bound per case and asserted <= 1 (the largest per family is recorded in DESIGN.md section 4.8)."""
import types

import numpy as np
import pytest
import torch
from transformers import BertConfig

import crf_entities_cases as X
import crf_llh_cases as K
import entity_cases as E
import params as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def tables(lmap, scheme):
    from mtvaf_amd.metrics import entity_device_tables, entity_tables
    return entity_device_tables(entity_tables(lmap, scheme), DEV)


def make_crf(start, end, trans):
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(start.numel(), batch_first=True).to(DEV)
    with torch.no_grad():
        crf.start_transitions.copy_(start)
        crf.end_transitions.copy_(end)
        crf.transitions.copy_(trans)
    return crf


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}


def check(what, res, ref, scheme, types_, max_entities):
    """entities / count exactly, log confidence by the rule, the derived fields of the dict"""
    r = host(res)
    want_e, want_c = X.expected(ref.chunks[scheme], types_, max_entities)
    assert r["count"].tolist() == want_c.tolist(), what
    assert r["entities"].tolist() == want_e.tolist(), what
    used = want_e[..., 0] >= 0
    lc = r["log_confidence"]
    assert np.isfinite(lc).all() and (lc[~used] == 0).all() and (r["confidence"][~used] == 0).all(), what
    assert np.allclose(r["confidence"][used], np.exp(lc[used]), rtol=1e-6, atol=0), what
    assert (lc <= ref.bound).all(), what  # a log probability
    q = X.ratio(f"{what} {scheme}", r["entities"], lc, ref)
    assert q <= 1.0, f"{what} {scheme}: err / bound = {q:.3f}"
    return int(used.sum())


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES + [(1, 512, 11, 1)], ids=lambda c: "B{}-S{}-C{}-x{}".format(*c))
def test_viterbi_tags_against_the_restatement(case):
    inp = X.inputs(case)
    em, _, mask, start, end, trans = inp
    lmap, crf = X.label_map(case[2]), make_crf(start, end, trans)
    em_d, mask_d = em.to(DEV), mask.to(DEV)
    first = crf.entities(em_d, mask_d, tables(lmap, "seqeval"), max_entities=64)
    tags = first["tags"].cpu().numpy()
    L = X.lengths_of(mask)
    assert first["lengths"].cpu().tolist() == L.tolist()
    assert all((tags[r, :L[r]] >= 0).all() and (tags[r, L[r]:] == -1).all() for r in range(case[0]))
    ref = X.reference(inp, tags, lmap, max_entities=64)
    for scheme in X.SCHEMES:
        t = tables(lmap, scheme)
        res = first if scheme == "seqeval" else crf.entities(em_d, mask_d, t, tags=first["tags"], max_entities=64)
        check(str(case), res, ref, scheme, t["types"], 64)


def test_given_tags_wild_ids_and_a_sentence_without_entity():
    """Random tags handed in (not Viterbi's), a tenth of them outside [0, C) -- they read as 0 --, sentence 0 all 'O'."""
    case = (5, 65, 11, 6)
    inp = X.inputs(case)
    em, tags, mask, start, end, trans = inp
    lmap, crf = X.label_map(11), make_crf(start, end, trans)
    tags = tags.clone()
    wild = torch.rand(tags.shape, generator=torch.Generator().manual_seed(9))
    tags[wild < 0.05] = -1
    tags[wild > 0.95] = 11 + 3
    tags[0] = lmap["O"]
    ref = X.reference(inp, tags.numpy(), lmap, max_entities=64)
    seen = 0
    for scheme in X.SCHEMES:
        t = tables(lmap, scheme)
        res = crf.entities(em.to(DEV), mask.to(DEV), t, tags=tags.to(DEV), max_entities=64)  # int64 tags cost a cast
        assert int(res["count"][0]) == 0 and bool((res["entities"][0] == -1).all())
        seen += check("given tags", res, ref, scheme, t["types"], 64)
    assert seen > 60


def test_more_sentences_than_waves_in_the_launch():
    inp = X.inputs(X.STRIDE_CASE)
    em, _, mask, start, end, trans = inp
    lmap, crf, t = X.label_map(2), make_crf(start, end, trans), tables(X.label_map(2), "seqeval")
    res = crf.entities(em.to(DEV), mask.to(DEV), t, max_entities=3)
    ref = X.reference(inp, res["tags"].cpu().numpy(), lmap, schemes=("seqeval",), max_entities=3)
    assert check("grid stride", res, ref, "seqeval", t["types"], 3) > 1000


# ---- 2. hand-built sentences -------------------------------------------------------------------------------------------------
def test_hand_built_sentences():
    """From entity_cases.long_skip_case: an entity with 79 non-kept columns inside it, one across columns 63 | 64, then an
    entity that is the whole sentence (column 0 kept) and a keep of all zeros."""
    lmap, S = E.label_map("a"), 256
    gold, _, _ = E.long_skip_case(lmap, S)
    b, i, x = lmap["B-NEU"], lmap["I-NEU"], lmap["X"]
    tags = np.stack([gold[0], gold[1], np.full(S, i), gold[1]]).astype(np.int32)
    tags[2, 0] = b
    keep = np.zeros((4, S), dtype=np.uint8)
    keep[:2, 1:] = tags[:2, 1:] != x
    keep[2] = 1
    mask = torch.ones(4, S, dtype=torch.uint8)
    mask[2, 200:] = 0
    gnr = torch.Generator().manual_seed(21)
    em = torch.randn(4, S, 11, generator=gnr) * 2
    start, end, trans = torch.rand(11, generator=gnr) - 0.5, torch.rand(11, generator=gnr) - 0.5, torch.rand(11, 11, generator=gnr) - 0.5
    inp = (em, None, mask, start, end, trans)
    crf = make_crf(start, end, trans)
    ref = X.reference(inp, tags, lmap, keep=keep, max_entities=8)
    for scheme in X.SCHEMES:
        t = tables(lmap, scheme)
        res = crf.entities(em.to(DEV), mask.to(DEV), t, tags=torch.from_numpy(tags).to(DEV), keep=torch.from_numpy(keep).to(DEV),
                           max_entities=8)
        check("hand-built", res, ref, scheme, t["types"], 8)
        got = host(res)["entities"]
        assert got[0, 0].tolist()[:2] == [10, 92] and got[0, 1].tolist()[:2] == [120, 120] and got[1, 0].tolist()[:2] == [60, 66]
        assert got[2, 0].tolist()[:2] == [0, 199] and int(res["count"][2]) == 1 and int(res["count"][3]) == 0


# ---- 3. truncation -----------------------------------------------------------------------------------------------------------
def test_truncation_keeps_the_first_chunks_and_the_true_count():
    lmap, S = E.label_map("a"), 130
    tags = np.full((2, S), lmap["O"], dtype=np.int32)
    tags[:, 1::2] = lmap["B-POS"]  # single-column entities at the odd columns
    mask = torch.ones(2, S, dtype=torch.uint8)
    mask[1, 4:] = 0                # sentence 1: columns 1 and 3
    gnr = torch.Generator().manual_seed(22)
    em = torch.randn(2, S, 11, generator=gnr)
    start, end, trans = torch.rand(11, generator=gnr) - 0.5, torch.rand(11, generator=gnr) - 0.5, torch.rand(11, 11, generator=gnr) - 0.5
    crf, t = make_crf(start, end, trans), tables(lmap, "seqeval")
    for max_entities in (2, 3, 64):
        ref = X.reference((em, None, mask, start, end, trans), tags, lmap, schemes=("seqeval",), max_entities=max_entities)
        res = crf.entities(em.to(DEV), mask.to(DEV), t, tags=torch.from_numpy(tags).to(DEV), max_entities=max_entities)
        check(f"max_entities={max_entities}", res, ref, "seqeval", t["types"], max_entities)
        r = host(res)
        assert r["count"].tolist() == [65, 2]
        assert r["entities"][0, :, 0].tolist() == list(range(1, 2 * max_entities, 2))
        if max_entities > 2:
            assert (r["entities"][1, 2:] == -1).all() and (r["log_confidence"][1, 2:] == 0).all()


# ---- 4. ties to the merged kernels -------------------------------------------------------------------------------------------
def test_whole_sentence_chunk_is_the_likelihood_and_single_column_chunk_the_marginal():
    lmap = E.label_map("a")
    em, _, mask, start, end, trans = X.inputs((5, 65, 11, 1))
    L = X.lengths_of(mask)
    crf, t = make_crf(start, end, trans), tables(lmap, "seqeval")
    em_d, mask_d = em.to(DEV), mask.to(DEV)
    # B I I ... I over every column of the sentence, column 0 kept: one chunk (0, L-1)
    tags = torch.full(mask.shape, lmap["I-NEG"], dtype=torch.long)
    tags[:, 0] = lmap["B-NEG"]
    ref_llh = K.make_reference((em, tags, mask, start, end, trans))
    ref = X.reference((em, None, mask, start, end, trans), tags.numpy(), lmap, keep=np.ones(mask.shape, dtype=np.uint8),
                      schemes=("seqeval",), max_entities=2)
    res = crf.entities(em_d, mask_d, t, tags=tags.to(DEV), keep=torch.ones_like(mask_d), max_entities=2)
    check("whole sentence", res, ref, "seqeval", t["types"], 2)
    assert host(res)["entities"][:, 0, :2].tolist() == [[0, int(n) - 1] for n in L]
    llh = crf(em_d, tags.to(DEV), mask_d, reduction="none").detach()
    err = float((res["log_confidence"][:, 0].double() - llh.double()).abs().max())
    print(f"crf-entities whole sentence vs llh kernel: err {err:.3e}, bounds {ref.bound:.3e} + {ref_llh.bound['llh']:.3e}")
    assert err <= ref.bound + ref_llh.bound["llh"]
    # B O B O ...: every odd column is a chunk of its own, its confidence the node marginal of that tag
    tags = torch.full(mask.shape, lmap["O"], dtype=torch.long)
    tags[:, 1::2] = lmap["B-POS"]
    res = crf.entities(em_d, mask_d, t, tags=tags.to(DEV), max_entities=64)
    marg = crf.marginals(em_d, mask_d).cpu()
    r, seen, err = host(res), 0, 0.0
    for s in range(5):
        cols = list(range(1, int(L[s]), 2))
        assert r["entities"][s, :len(cols), 0].tolist() == cols and r["entities"][s, :len(cols), 1].tolist() == cols
        for k, c in enumerate(cols):
            err = max(err, abs(float(r["confidence"][s, k]) - float(marg[s, c, lmap["B-POS"]])))
            seen += 1
    print(f"crf-entities single column vs marginals kernel: err {err:.3e}, bound {ref_llh.bound['marg']:.3e}")
    assert seen > 40 and err <= ref_llh.bound["marg"]


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------
def small_call():
    em, _, mask, start, end, trans = X.inputs((3, 16, 2, 1))
    lmap = X.label_map(2)
    crf, t = make_crf(start, end, trans), tables(lmap, "seqeval")
    return crf, t, em.to(DEV), mask.to(DEV)


def test_bad_arguments_return_the_code_and_launch_nothing():
    from mtvaf_amd import hip
    crf, t, em, mask = small_call()
    tags, _ = crf.decode_packed(em, mask)
    ents = torch.full((3, 4, 3), 12345, dtype=torch.int32, device=DEV)
    lc = torch.full((3, 4), 7.5, device=DEV)
    cnt = torch.full((3,), -7, dtype=torch.int32, device=DEV)

    def rc(S=16, C=2, ldt=16, max_entities=4, n_types=None):
        return hip.lib().mtvaf_crf_entities(
            em.data_ptr(), mask.data_ptr(), tags.data_ptr(), ldt, None, crf.start_transitions.data_ptr(),
            crf.end_transitions.data_ptr(), crf.transitions.data_ptr(), t["start"].data_ptr(), t["end"].data_ptr(),
            t["type_of"].data_ptr(), t["n_types"] if n_types is None else n_types, ents.data_ptr(), lc.data_ptr(), cnt.data_ptr(),
            3, S, C, max_entities, hip._st())
    assert rc(S=513) == -1 and rc(C=65) == -1 and rc(ldt=15) == -1
    assert rc(max_entities=0) == -3 and rc(max_entities=65) == -3 and rc(n_types=4) == -3
    torch.cuda.synchronize()
    assert bool((ents == 12345).all()) and bool((lc == 7.5).all()) and bool((cnt == -7).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((ents == 12345).any()) and not bool((lc == 7.5).any()) and not bool((cnt == -7).any())
    with pytest.raises(ValueError):
        crf.entities(em, mask, t, max_entities=65)
    with pytest.raises(ValueError):
        crf.entities(em, mask, t, tags=tags[:, :15])


def test_strided_tags_are_read_in_place_and_a_repeat_call_overwrites_everything():
    from mtvaf_amd import hip
    crf, t, em, mask = small_call()
    first = crf.entities(em, mask, t, max_entities=5)
    wide = torch.full((3, 16 + 7), 1, dtype=torch.int32, device=DEV)  # a tag that would chunk differently behind column S
    wide[:, :16] = first["tags"]
    view = wide[:, :16]
    assert view.stride(0) == 23 and not view.is_contiguous()
    again = crf.entities(em, mask, t, tags=view, max_entities=5)
    assert again["tags"].data_ptr() == wide.data_ptr()
    for k in ("entities", "log_confidence", "count"):
        assert torch.equal(first[k], again[k]), k
    out = (torch.full((3, 5, 3), 12345, dtype=torch.int32, device=DEV), torch.full((3, 5), float("nan"), device=DEV),
           torch.full((3,), -7, dtype=torch.int32, device=DEV))
    par = (crf.start_transitions.data, crf.end_transitions.data, crf.transitions.data)
    got = hip.crf_entities(em, mask, view, None, *par, t["start"], t["end"], t["type_of"], t["n_types"], 5, out=out)
    assert got[0] is out[0]
    for k, o in zip(("entities", "log_confidence", "count"), out):
        assert torch.equal(first[k], o), k  # (bit for bit: a NaN left behind would not compare equal)
    assert int(first["count"].sum()) > 0 and bool((first["entities"] == -1).any())


# ---- 6. capture and replay ---------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_emissions():
    """One capture of Viterbi + entities in a single-stream graph, replayed after the emissions changed in place: no host sync, no
    allocation that the graph's pool does not own."""
    case = (3, 65, 11, 1)
    inp = X.inputs(case)
    em, _, mask, start, end, trans = inp
    em2 = X.inputs((3, 65, 11, 6))[0]
    lmap, crf, t = X.label_map(11), make_crf(start, end, trans), tables(X.label_map(11), "seqeval")
    buf, mask_d = em.to(DEV).clone(), mask.to(DEV)
    crf.entities(buf, mask_d, t, max_entities=64)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crf.entities(buf, mask_d, t, max_entities=64)
    seen = []
    for emissions in (em, em2):
        buf.copy_(emissions)
        graph.replay()
        ref = X.reference((emissions,) + inp[1:], out["tags"].cpu().numpy(), lmap, schemes=("seqeval",), max_entities=64)
        check("replay", out, ref, "seqeval", t["types"], 64)
        seen.append(out["entities"].cpu().clone())
    assert not torch.equal(seen[0], seen[1])


# ---- 7. the model ------------------------------------------------------------------------------------------------------------
LABELS = E.SET_A
LABEL_MAP = {label: i for i, label in enumerate(LABELS, 1)}


def tiny_model(use_prefix, **kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=use_prefix, vao=use_prefix, noauxloss=False,
                                 use_probe=False, n_gpu=1, alpha=0.5, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV,
                                 resnet_root=None, use_152=False, **kw)
    args.bert_config = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                                  num_attention_heads=cfg.heads, intermediate_size=cfg.inter,
                                  max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.eps,
                                  hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    m = TVNetSAModel2(LABELS, None, args).to(DEV)
    with torch.no_grad():  # an untrained head decodes mostly one tag: spread the emissions so the batch holds entities
        m.fc.weight.mul_(40.0)
    return cfg, m


@pytest.mark.parametrize("use_prefix", [False, True])
def test_predict(use_prefix):
    from mtvaf_amd import engine
    from mtvaf_amd.metrics import entities_to_lists, structural_labels
    cfg, m = tiny_model(use_prefix, max_entities=16)
    B, S = 6, 32
    ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 51, B, S, lo_id=5))
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt)
    extra = {}
    if use_prefix:
        g = torch.Generator().manual_seed(52)
        kw.update(images=torch.rand(B, 3840, 2, 2, generator=g).to(DEV), aux_imgs=torch.rand(B, 3, 3840, 2, 2, generator=g).to(DEV))
        extra = dict(imagelabel=torch.softmax(torch.randn(B, 2089, generator=g), -1).to(DEV))

    def train_step():
        torch.manual_seed(5)
        engine.RNG.offset = 1000
        out = m.train()(labels=labels, **kw, **extra)
        return out.loss.detach().clone(), list(out.logits)

    loss0, tags0 = train_step()
    offset = engine.RNG.offset
    res = m.predict(**kw)                     # from train mode
    assert m.training and engine.RNG.offset == offset and all(not p.requires_grad or p.grad is None for p in m.parameters())
    loss1, tags1 = train_step()
    assert torch.equal(loss0, loss1) and tags0 == tags1, "predict left state behind"

    m.eval()
    with torch.no_grad():
        fwd = m(**kw, **extra)
    res2 = m.predict(**kw)
    assert not m.training
    L = X.lengths_of(mask.cpu().numpy())
    tags = res["tags"].cpu().numpy()
    assert [tags[r, :L[r]].tolist() for r in range(B)] == list(fwd.logits)
    for k in ("tags", "entities", "log_confidence", "confidence", "count"):
        assert torch.equal(res[k], res2[k]), k

    # CRF.entities on the same emissions, the restatement on the same tags
    cap = {}
    hook = m.bert.register_forward_hook(lambda mod, inp, out: cap.update(h=out["last_hidden_state"]))
    with torch.no_grad():
        m(**kw, **extra)
    hook.remove()
    em = engine.LinearFunction.apply(cap["h"], m.fc.weight, m.fc.bias, False).detach()
    structural = [LABEL_MAP.get(n, 0) for n in structural_labels(LABEL_MAP)]
    assert sorted(structural) == [0, LABEL_MAP["X"], LABEL_MAP["[CLS]"], LABEL_MAP["[SEP]"]]
    run = np.zeros((B, S), dtype=bool)
    run[:, 1:] = np.logical_and.accumulate(mask.cpu().numpy()[:, 1:] != 0, axis=1)
    keep = run & ~np.isin(np.clip(tags, 0, 10), structural)
    t = tables(LABEL_MAP, "seqeval")
    direct = m.crf.entities(em, mask.to(torch.uint8), t, tags=res["tags"], keep=torch.from_numpy(keep).to(DEV), max_entities=16)
    for k in ("entities", "log_confidence", "confidence", "count"):
        assert torch.equal(res[k], direct[k]), k
    assert res["types"] == t["types"] and tuple(res["entities"].shape) == (B, 16, 3)
    inp = (em.cpu(), None, mask.cpu().to(torch.uint8), m.crf.start_transitions.detach().cpu(),
           m.crf.end_transitions.detach().cpu(), m.crf.transitions.detach().cpu())
    ref = X.reference(inp, tags, LABEL_MAP, keep=keep, schemes=("seqeval",), max_entities=16)
    assert check("predict", res, ref, "seqeval", t["types"], 16) >= 3, "the batch holds too few entities to show anything"
    lists = entities_to_lists(res, res["types"])
    assert [len(x) for x in lists] == np.minimum(res["count"].cpu().numpy(), 16).tolist()
    first = next(x[0] for x in lists if x)
    assert set(first) == {"start", "end", "type", "confidence"} and first["type"] in ("NEU", "POS", "NEG") and 0 < first["confidence"] <= 1

    # word_mask: only its columns take part
    wm = torch.zeros(B, S, dtype=torch.long)
    wm[:, 1::2] = 1
    res3 = m.predict(word_mask=wm.to(DEV), **kw)
    keep3 = keep & (wm.numpy() != 0)
    ref3 = X.reference(inp, tags, LABEL_MAP, keep=keep3, schemes=("seqeval",), max_entities=16)
    check("predict word_mask", res3, ref3, "seqeval", t["types"], 16)
    assert not torch.equal(res3["entities"], res["entities"])

    # args.entity_scheme picks the tables
    m.args.entity_scheme = "reference"
    res4 = m.predict(**kw)
    ref4 = X.reference(inp, tags, LABEL_MAP, keep=keep, schemes=("reference",), max_entities=16)
    t4 = tables(LABEL_MAP, "reference")
    assert res4["types"] == t4["types"]
    check("predict reference scheme", res4, ref4, "reference", t4["types"], 16)
