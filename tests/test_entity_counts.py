"""Entity counting, the parts that need no GPU: the sequential restatement of the rule (tests/entity_cases.py) against the counts the
reference's own get_chunks / evaluate / evaluate_each_class gave (tests/golden/entity_chunks.npz), the table builder of
`mtvaf_amd.metrics` against hand-derived chunk lists and against the restatement's predicates, and `EntityScorer.compute`'s
arithmetic from a hand-filled counter."""
import os

import numpy as np
import pytest
import torch

import abi_header
import entity_cases as E

G = os.path.join(os.path.dirname(__file__), "golden")


def fixture():
    return dict(np.load(os.path.join(G, "entity_chunks.npz")))


def fixture_counter(fx, s, types):
    """The fixture's reference-made counts of label set s laid out as the counter of a scorer with these types."""
    per = {str(t): [int(v) for v in row] for t, row in zip(fx[f"{s}_types"], fx[f"{s}_counts"]) if row.any()}
    return E.counter(types, (per, int(fx[f"{s}_tokens"][0]), int(fx[f"{s}_tokens"][1])))


@pytest.mark.parametrize("s", ["a", "b"])
def test_restatement_equals_the_reference_counts(s):
    fx = fixture()
    per, equal, kept = E.restate(E.label_map(s), "reference", fx[f"{s}_gold"], fx[f"{s}_pred"], fx[f"{s}_mask"])
    want = {str(t): [int(v) for v in row] for t, row in zip(fx[f"{s}_types"], fx[f"{s}_counts"]) if row.any()}
    assert {t: v for t, v in per.items() if any(v)} == want
    assert [equal, kept] == fx[f"{s}_tokens"].tolist()
    assert kept > 500 and sum(v[2] for v in want.values()) > 100  # the fixture is not degenerate


def table_chunks(tab, ids):
    """Chunks of one sentence of label ids read off the TABLES of metrics.entity_tables (what the kernel is handed)."""
    C, out, begin = tab["C"], [], None
    for j, cur in enumerate(ids):
        prev = ids[j - 1] if j else C
        nxt = ids[j + 1] if j + 1 < len(ids) else C
        if tab["start"][prev, cur]:
            begin = j
        if tab["end"][cur, nxt]:
            out.append((tab["types"][tab["type_of"][cur]], begin, j))
    return out


NAMES = ["O", "B-PER", "I-PER", "I-LOC", "I-ORG", "B-POS", "I-POS", "E-POS", "X", "[CLS]", "[SEP]"]
KNOWN = [  # names, seqeval chunks, reference chunks
    (["B-PER", "I-PER", "O", "I-LOC"], [("PER", 0, 1), ("LOC", 3, 3)], None),
    (["B-PER", "B-PER"], [("PER", 0, 0), ("PER", 1, 1)], None),
    (["I-PER", "I-ORG"], [("PER", 0, 0), ("ORG", 1, 1)], None),
    (["B-POS", "E-POS", "I-POS"], [("POS", 0, 1), ("POS", 2, 2)], [("POS", 0, 2)]),
    (["O", "X", "B-POS"], [("_", None, 1), ("POS", 2, 2)], [("X", 1, 1), ("POS", 2, 2)]),
    (["O", "PAD"], [("AD", 1, 1)], [("PAD", 1, 1)]),
]


@pytest.mark.parametrize("names,seqeval,reference", KNOWN)
def test_known_answers_of_both_schemes(names, seqeval, reference):
    from mtvaf_amd.metrics import entity_tables
    lmap = {n: i for i, n in enumerate(NAMES, 1)}
    ids = [lmap.get(n, 0) for n in names]  # "PAD" is id 0
    for scheme, want in (("seqeval", seqeval), ("reference", reference or seqeval)):
        assert E.name_chunks(scheme, names) == want, scheme
        assert table_chunks(entity_tables(lmap, scheme), ids) == want, scheme


@pytest.mark.parametrize("scheme", ["seqeval", "reference"])
@pytest.mark.parametrize("s", ["a", "b", "c"])
def test_tables_are_the_predicates(s, scheme):
    from mtvaf_amd.metrics import entity_tables
    lmap = E.label_map(s)
    tab, labs = entity_tables(lmap, scheme), E.labels_of(lmap) + [E.BOUNDARY]
    C = tab["C"]
    assert C == len(labs) - 1 == {"a": 11, "b": 16, "c": 64}[s] and tab["names"] == [n for n, _ in labs[:C]]
    assert tab["start"].shape == tab["end"].shape == (C + 1, C + 1) and len(tab["types"]) <= C + 1
    for p in range(C + 1):
        for c in range(C + 1):
            assert bool(tab["start"][p, c]) == bool(E.is_start(scheme, labs[p], labs[c])), (labs[p], labs[c])
            assert bool(tab["end"][p, c]) == bool(E.is_end(scheme, labs[p], labs[c])), (labs[p], labs[c])
    assert [tab["types"][t] for t in tab["type_of"]] == [E.type_name(scheme, lab) for lab in labs]
    assert tab["gold_skip"].tolist() == [int(n in E.SKIP) for n, _ in labs[:C]]
    want_primary = {"a": {"NEU", "POS", "NEG"}, "b": {"POS", "NEG", "NEU"} | ({"Q"} if scheme == "seqeval" else set()),
                    "c": {f"T{t:02d}" for t in range(15)}}[s]
    assert {t for t, p in zip(tab["types"], tab["primary"]) if p} == want_primary


def test_table_builder_rejects_bad_input():
    from mtvaf_amd.metrics import EntityScorer, entity_tables
    with pytest.raises(ValueError, match="scheme"):
        entity_tables(E.label_map("a"), "iob3")
    with pytest.raises(ValueError, match="'O'"):
        entity_tables({"B-X": 1, "I-X": 2})
    with pytest.raises(ValueError, match="64"):
        EntityScorer({**E.label_map("c"), "B-EXTRA": 64}, device="cpu")


def test_compute_arithmetic_from_a_hand_filled_counter():
    from mtvaf_amd.metrics import EntityScorer
    sc = EntityScorer(E.label_map("a"), scheme="seqeval", device="cpu")
    assert sc.counts.dtype == torch.int64 and sc.counts.numel() == len(sc.types) * 3 + 2 and not sc.counts.any()
    empty = sc.compute()
    assert set(empty) == {"NEU", "POS", "NEG", "micro", "macro", "weighted", "token_accuracy"}
    assert empty["token_accuracy"] == 0.0 and empty["POS"]["f1"] == 0.0 and empty["micro"]["precision"] == 0.0
    assert empty["macro"]["f1"] == 0.0 and empty["weighted"]["recall"] == 0.0

    def fill(name, predicted, gold, correct):
        t = sc.types.index(name)
        sc.counts[3 * t:3 * t + 3] = torch.tensor([predicted, gold, correct])
    fill("NEU", 4, 8, 2)    # p 0.5   r 0.25  f 1/3
    fill("POS", 10, 5, 5)   # p 0.5   r 1     f 2/3
    fill("NEG", 0, 3, 0)    # p 0 (0 / 0)  r 0  f 0
    fill("_", 2, 0, 0)      # a predicted "X" chunk: listed because it has counts
    sc.counts[-2:] = torch.tensor([30, 40])
    got = sc.compute()
    assert set(got) == {"NEU", "POS", "NEG", "_", "micro", "macro", "weighted", "token_accuracy"}
    assert got["NEU"] == dict(predicted=4, support=8, correct=2, precision=0.5, recall=0.25, f1=2 * 0.5 * 0.25 / 0.75)
    assert got["POS"] == dict(predicted=10, support=5, correct=5, precision=0.5, recall=1.0, f1=2 * 0.5 / 1.5)
    assert got["NEG"] == dict(predicted=0, support=3, correct=0, precision=0.0, recall=0.0, f1=0.0)
    assert got["_"] == dict(predicted=2, support=0, correct=0, precision=0.0, recall=0.0, f1=0.0)
    p, r = 7 / 16, 7 / 16
    assert got["micro"] == dict(predicted=16, support=16, correct=7, precision=p, recall=r, f1=2 * p * r / (p + r))
    f_neu, f_pos = got["NEU"]["f1"], got["POS"]["f1"]
    assert got["macro"] == dict(support=16, precision=(0.5 + 0.5) / 4, recall=(0.25 + 1.0) / 4, f1=(f_neu + f_pos) / 4)
    assert got["weighted"] == dict(support=16, precision=(0.5 * 8 + 0.5 * 5) / 16, recall=(0.25 * 8 + 1.0 * 5) / 16,
                                   f1=(f_neu * 8 + f_pos * 5) / 16)
    assert got["token_accuracy"] == 0.75
    sc.reset()
    assert not sc.counts.any() and sc.compute() == empty
    sc.all_reduce()  # no process group: nothing happens


def test_entity_counts_is_exported_and_rejects_shapes_beyond_its_limits():
    from mtvaf_amd import hip
    assert "mtvaf_entity_counts" in hip.exported_symbols()
    f = hip.lib().mtvaf_entity_counts
    assert f.argtypes == hip._SIGS["mtvaf_entity_counts"][1] == abi_header.signature("mtvaf_entity_counts")[1]
    assert f(None, 513, None, None, None, None, None, None, 2, 513, 11, 4, None, None) == -1   # S = 513
    assert f(None, 16, None, None, None, None, None, None, 2, 16, 65, 4, None, None) == -1     # C = 65
    assert f(None, 15, None, None, None, None, None, None, 2, 16, 11, 4, None, None) == -1     # tags narrower than the labels
    assert f(None, 16, None, None, None, None, None, None, 2, 16, 11, 13, None, None) == -3    # more types than labels + boundary
    z = torch.zeros
    with pytest.raises(ValueError, match="S=513"):
        hip.entity_counts(z(2, 513, dtype=torch.int32), z(2, 513, dtype=torch.int64), z(2, 513, dtype=torch.uint8), z(144), z(144),
                          z(12), z(11), 4, z(14))
    with pytest.raises(ValueError, match="C=65"):
        hip.entity_counts(z(2, 16, dtype=torch.int32), z(2, 16, dtype=torch.int64), z(2, 16, dtype=torch.uint8), z(66 * 66),
                          z(66 * 66), z(66), z(65), 4, z(14))
