"""CPU side of the tagger-inference tests: the references of tests/crf_entities_cases.py against brute force, the host helpers of
`mtvaf_amd.metrics`, and the declaration of `mtvaf_crf_entities` (header, ctypes mirror, exported symbol)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import crf_entities_cases as X
import crf_llh_cases as K
import crf_wide_cases as W
import entity_cases as E


@pytest.mark.parametrize("case", [(3, 4, 5, 76, (4, 2, 1)), (2, 3, 2, 79, (3, 1)), (1, 6, 3, 80, (6,))])
def test_constrained_partition_reference_equals_enumeration(case):
    """Every segment b..e of every sentence, tags fixed to the drawn ones: the float64 reference of the cases module equals the
    sum over all C^L paths that agree with the tags on the segment, to 1e-10."""
    B, S, C, seed, lengths = case
    em, tags, mask, start, end, trans = W.crf_inputs(B, S, C, seed, lengths=list(lengths))
    segments = [(r, b, e) for r in range(B) for b in range(lengths[r]) for e in range(b, lengths[r])]
    got, logz = X.log_posteriors(em, mask, start, end, trans, tags, segments, torch.float64)
    for (r, b, e), g in zip(segments, got.tolist()):
        want = X.bruteforce_log_posterior(em, mask, start, end, trans, tags, r, b, e)
        assert abs(g - want) <= 1e-10, (r, b, e, g, want)
        assert g <= 1e-12
    assert torch.allclose(logz, K.bruteforce(em, tags, mask, start, end, trans)[1], rtol=0, atol=1e-10)
    # the whole sentence is the likelihood of the path, a single column the node marginal
    llh, _, marg = K.bruteforce(em, tags, mask, start, end, trans)
    for r in range(B):
        whole = got[segments.index((r, 0, lengths[r] - 1))]
        assert abs(float(whole) - float(llh[r])) <= 1e-10
        one = got[segments.index((r, 0, 0))]
        assert abs(float(one.exp()) - float(marg[r, 0, tags[r, 0]])) <= 1e-10


def test_float32_reference_meets_the_rule_and_is_finite():
    """The rule's bound is never spent on a case the float32 reference itself misses (it cannot: by construction), the references
    hold no NaN / inf with -inf emissions in them, and the cases are not empty."""
    seen = 0
    for case in [(3, 65, 11, 1), (3, 65, 11, 6), (3, 16, 2, 1), (5, 65, 1, 1)]:
        inp = X.inputs(case)
        tags = X.sanitised(inp[1], case[2]).numpy()
        ref = X.reference(inp, tags, X.label_map(case[2]))
        for seg in ref.segments:
            assert abs(ref.ref32[seg] - ref.ref64[seg]) <= ref.bound and ref.ref64[seg] <= 1e-9
        seen += len(ref.segments)
    assert seen > 50


def test_reference_chunker_maps_kept_positions_back_to_columns():
    lmap = E.label_map("a")
    o, b, i, x = lmap["O"], lmap["B-POS"], lmap["I-POS"], lmap["X"]
    tags = np.array([[lmap["[CLS]"], b, x, x, i, o, b, lmap["[SEP]"]],
                     [lmap["[CLS]"], i, i, o, o, o, o, o]])
    mask = np.ones((2, 8), dtype=np.uint8)
    mask[1, 4:] = 0
    keep = (tags != x) & (tags != lmap["[CLS]"]) & (tags != lmap["[SEP]"])
    got = X.chunks_of(lmap, "seqeval", tags, mask, keep)
    assert got == [[(1, 4, "POS"), (6, 6, "POS")], [(1, 2, "POS")]]
    # the "reference" scheme opens a chunk at an I that follows O too; without a keep, X takes part and splits the first entity
    assert X.chunks_of(lmap, "reference", tags, mask, keep) == got
    assert X.chunks_of(lmap, "reference", tags, mask)[0][:2] == [(1, 1, "POS"), (2, 3, "X")]
    ents, count = X.expected(got, ["O", "POS"], 1)
    assert ents.tolist() == [[[1, 4, 1]], [[1, 2, 1]]] and count.tolist() == [2, 1]


def test_structural_labels():
    from mtvaf_amd.metrics import structural_labels
    assert structural_labels(E.label_map("a")) == ("PAD", "X", "[CLS]", "[SEP]")
    assert structural_labels(E.label_map("b")) == ("PAD", "EQ", "[CLS]", "[SEP]")
    assert structural_labels(E.label_map("c")) == ("PAD", "[CLS]", "X", "[SEP]")
    assert structural_labels({"O": 1, "PAD": 0, "B-": 2, "-x": 3}) == ("PAD", "B-", "-x")


def test_entities_to_lists():
    from mtvaf_amd.metrics import entities_to_lists
    ents = torch.full((3, 2, 3), -1, dtype=torch.int32)
    ents[0, 0] = torch.tensor([1, 3, 2])
    ents[0, 1] = torch.tensor([5, 5, 1])
    ents[2, 0] = torch.tensor([2, 2, 1])
    ents[2, 1] = torch.tensor([4, 9, 2])
    conf = torch.tensor([[0.75, 0.5], [0.0, 0.0], [0.125, 1.0]])
    result = dict(entities=ents, confidence=conf, count=torch.tensor([2, 0, 5], dtype=torch.int32))  # 5 found, 2 stored
    got = entities_to_lists(result, ["O", "POS", "NEG"])
    assert got == [[dict(start=1, end=3, type="NEG", confidence=0.75), dict(start=5, end=5, type="POS", confidence=0.5)], [],
                   [dict(start=2, end=2, type="POS", confidence=0.125), dict(start=4, end=9, type="NEG", confidence=1.0)]]


def test_entity_device_tables_keep_the_layout_of_entity_tables():
    from mtvaf_amd.metrics import entity_device_tables, entity_tables
    t = entity_tables(E.label_map("a"), "seqeval")
    d = entity_device_tables(t, "cpu")
    assert d["start"].dtype == d["end"].dtype == torch.uint8 and d["type_of"].dtype == torch.int32
    assert d["start"].tolist() == t["start"].reshape(-1).tolist() and d["end"].tolist() == t["end"].reshape(-1).tolist()
    assert d["type_of"].tolist() == t["type_of"].tolist() and d["n_types"] == len(t["types"]) and d["C"] == 11
    assert entity_device_tables(d, "cpu") is d


# ---- the declaration ---------------------------------------------------------------------------------------------------------
def test_header_binding_and_export_agree():
    from mtvaf_amd import hip
    from mtvaf_amd.build import build_library
    res, args = hip._SIGS["mtvaf_crf_entities"]
    assert (res, list(args)) == abi_header.signature("mtvaf_crf_entities") and res is ctypes.c_int
    assert [name for _, name in abi_header.prototype("mtvaf_crf_entities")[2]] == [
        "emissions", "mask", "tags", "ldt", "keep", "start", "end", "trans", "start_tab", "end_tab", "type_of", "n_types", "ents",
        "log_conf", "count", "B", "S", "C", "max_entities", "stream"]
    assert "mtvaf_crf_entities" in hip.exported_symbols()
    assert hasattr(ctypes.CDLL(build_library(verbose=False)), "mtvaf_crf_entities")
    assert "crf_entities.hip" in __import__("mtvaf_amd.build", fromlist=["SOURCES"]).SOURCES
    comment = abi_header.comment_before("mtvaf_crf_entities")
    for word in ("models/bert_model.py:511", "modules/eval_metrics.py::get_chunks", "prefix", "holes"):
        assert word in comment.replace("PREFIX", "prefix"), word


def test_argument_checks_come_before_any_launch():
    """The shape / argument errors are decided on the host: with null pointers and no GPU the call returns the code."""
    from mtvaf_amd import hip
    fn = hip.lib().mtvaf_crf_entities

    def rc(B=2, S=8, C=5, ldt=8, n_types=3, max_entities=4):
        return fn(None, None, None, ldt, None, None, None, None, None, None, None, n_types, None, None, None, B, S, C,
                  max_entities, None)
    assert rc(S=513) == -1 and rc(S=0) == -1 and rc(C=65) == -1 and rc(C=0) == -1 and rc(ldt=7) == -1 and rc(B=0) == -1
    assert rc(max_entities=0) == -3 and rc(max_entities=65) == -3 and rc(n_types=0) == -3 and rc(n_types=7) == -3


def test_wrapper_raises_value_error_for_bad_shapes():
    from mtvaf_amd import hip
    em = torch.zeros(2, 8, 5)
    mask, tags = torch.ones(2, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.int32)
    par = (torch.zeros(5), torch.zeros(5), torch.zeros(5, 5))
    tab = (torch.zeros(36, dtype=torch.uint8), torch.zeros(36, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32))

    def call(em=em, mask=mask, tags=tags, keep=None, par=par, tab=tab, n_types=2, max_entities=4):
        return hip.crf_entities(em, mask, tags, keep, *par, *tab, n_types, max_entities)
    for kw in (dict(em=torch.zeros(2, 513, 5)), dict(em=torch.zeros(2, 8, 65)), dict(max_entities=0), dict(max_entities=65),
               dict(n_types=7), dict(tags=tags[:, :7]), dict(tags=tags[:1]), dict(mask=mask[:, :7]), dict(keep=mask[:1]),
               dict(tags=torch.zeros(2, 16, dtype=torch.int32)[:, ::2]), dict(em=torch.zeros(8, 5)),
               dict(tab=(tab[0][:25], tab[1], tab[2])), dict(par=(par[0], par[1], torch.zeros(4, 4)))):
        with pytest.raises(ValueError):
            call(**kw)
