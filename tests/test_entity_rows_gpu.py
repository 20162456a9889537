"""Per-row entity counts on the MI355X: `mtvaf_entity_counts_rows` / `metrics.sentence_f1_cost` against the sequential restatement
of the chunk rule (tests/entity_cases.py) on every row alone, and against `mtvaf_entity_counts` -- the existing kernel -- called on
that single row.  Every comparison of counts is exact integer equality."""
import numpy as np
import pytest
import torch

import entity_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCHEMES = ("seqeval", "reference")
B, K = 3, 4


def tables(s, scheme):
    from mtvaf_amd.metrics import entity_device_tables, entity_tables
    return entity_device_tables(entity_tables(E.label_map(s), scheme), DEV)


def hypotheses(s, S, mask_kind, seed):
    """gold [B,S], K hypotheses per sentence [B,K,S] (-1 behind the mask), mask [B,S]: hypothesis 0 is the gold row itself"""
    lmap, rng = E.label_map(s), np.random.default_rng(seed)
    gold, pred0, mask = E.make_case(rng, lmap, B, S, mask_kind, "equal", 0.3)
    hyp = [pred0]
    for k in range(1, K):
        _, p, _ = E.make_case(np.random.default_rng(seed + k), lmap, B, S, mask_kind, ("mixed", "uniform", "wild")[k - 1], 0.3)
        agree = np.random.default_rng(seed + 10 + k).random((B, S)) < 0.5
        p = np.where(agree, gold, p)
        hyp.append(np.where(mask.astype(bool), p, -1).astype(np.int32))
    return gold, np.stack(hyp, axis=1), mask


def long_case(s):
    """entity_cases.long_skip_case (S = 256) as K hypotheses: its prediction, its gold, and two shifted copies"""
    gold, pred, mask = E.long_skip_case(E.label_map(s), 256)
    hyp = np.stack([pred, gold.astype(np.int32), np.roll(pred, 1, axis=1), np.roll(pred, -1, axis=1)], axis=1)
    return gold, hyp, mask


def want_rows(s, scheme, gold, hyp, mask):
    out = np.zeros(hyp.shape[:2] + (3,), dtype=np.int64)
    for b in range(hyp.shape[0]):
        for k in range(hyp.shape[1]):
            per, _, _ = E.restate(E.label_map(s), scheme, gold[b:b + 1], hyp[b, k][None], mask[b:b + 1])
            out[b, k] = np.sum(list(per.values()), axis=0) if per else 0
    return out


def rows_of(t, gold, hyp, mask):
    from mtvaf_amd import hip
    Bn, Kn, S = hyp.shape
    out = torch.full((Bn * Kn, 3), -7, dtype=torch.int32, device=DEV)  # junk: every element must be overwritten
    hip.entity_counts_rows(torch.from_numpy(hyp).to(DEV).view(Bn * Kn, S), torch.from_numpy(gold).to(DEV), torch.from_numpy(mask).to(DEV),
                           t["start"], t["end"], t["type_of"], t["gold_skip"], t["n_types"], group=Kn, out=out)
    return out.cpu().numpy().reshape(Bn, Kn, 3)


def global_counts(t, gold, pred, mask):
    """`mtvaf_entity_counts` on a batch -> (predicted, gold, correct) summed over the types"""
    from mtvaf_amd import hip
    counts = torch.zeros(t["n_types"] * 3 + 2, dtype=torch.int64, device=DEV)
    hip.entity_counts(torch.from_numpy(pred.copy()).to(DEV), torch.from_numpy(gold.copy()).to(DEV),  # (copies: plain row strides)
                      torch.from_numpy(mask.copy()).to(DEV), t["start"], t["end"], t["type_of"], t["gold_skip"], t["n_types"], counts)
    return counts.cpu().numpy()[:-2].reshape(-1, 3).sum(0)


CASES = [(s, mk) for s in ("a", "c") for mk in ("ragged", "col0")]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("s,mask_kind", CASES + [("a", "long"), ("c", "long")])
def test_rows_against_the_restatement_and_the_existing_kernel(s, mask_kind, scheme):
    gold, hyp, mask = long_case(s) if mask_kind == "long" else hypotheses(s, 16, mask_kind, 21)
    t = tables(s, scheme)
    got = rows_of(t, gold, hyp, mask)
    assert got.tolist() == want_rows(s, scheme, gold, hyp, mask).tolist()
    for b in range(hyp.shape[0]):  # the existing kernel on that single row: a second reference
        for k in range(hyp.shape[1]):
            assert got[b, k].tolist() == global_counts(t, gold[b:b + 1], hyp[b, k][None], mask[b:b + 1]).tolist(), (b, k)
    if mask_kind == "col0":
        assert not got.any()
    else:  # (the gold side of a row does not depend on its hypothesis)
        assert got[..., 2].any() and (got[..., 1] == got[:, :1, 1]).all()
    # the column sums over all rows: one batched call of the existing kernel, every row against its own gold row (group = 1)
    Bn, Kn, S = hyp.shape
    flat_gold, flat_mask = np.repeat(gold, Kn, axis=0), np.repeat(mask, Kn, axis=0)
    assert got.reshape(-1, 3).sum(0).tolist() == global_counts(t, flat_gold, hyp.reshape(Bn * Kn, S), flat_mask).tolist()
    from mtvaf_amd import hip
    ones = hip.entity_counts_rows(torch.from_numpy(hyp).to(DEV).view(Bn * Kn, S), torch.from_numpy(flat_gold).to(DEV),
                                  torch.from_numpy(flat_mask).to(DEV), t["start"], t["end"], t["type_of"], t["gold_skip"],
                                  t["n_types"], group=1)
    assert ones.cpu().numpy().reshape(Bn, Kn, 3).tolist() == got.tolist()


def test_sentence_f1_cost_follows_from_the_counts():
    from mtvaf_amd.metrics import entity_tables, sentence_f1_cost
    gold, hyp, mask = hypotheses("a", 16, "ragged", 33)
    hyp[2, 1] = np.where(mask[2].astype(bool), E.label_map("a")["O"], -1)  # predicts nothing
    args = (torch.from_numpy(hyp).to(DEV), torch.from_numpy(gold).to(DEV), torch.from_numpy(mask.astype(np.int64)).to(DEV))
    cost, rows = sentence_f1_cost(*args, tables("a", "seqeval"), return_counts=True)
    again = sentence_f1_cost(*args, entity_tables(E.label_map("a"), "seqeval"))  # the host dict of entity_tables
    want = want_rows("a", "seqeval", gold, hyp, mask)
    assert rows.cpu().numpy().tolist() == want.tolist()
    p, g, c = (want[..., i].astype(np.float64) for i in range(3))
    f1 = np.where(p + g > 0, 2 * c / np.maximum(p + g, 1), 1.0)
    assert cost.dtype == torch.float32 and tuple(cost.shape) == (B, K) and torch.equal(cost, again)
    assert np.abs(cost.cpu().numpy() - (1 - f1)).max() <= 2.0 ** -23
    assert float(cost.min()) >= 0.0 and float(cost.max()) <= 1.0
    assert want[2, 1, 0] == 0 and float(cost[2, 1]) == (1.0 if want[2, 1, 1] else 0.0)
    # nothing to find and nothing found: cost 0
    o = np.full((1, 1, 16), E.label_map("a")["O"], dtype=np.int32)
    none = sentence_f1_cost(torch.from_numpy(o).to(DEV), torch.from_numpy(o[0].astype(np.int64)).to(DEV),
                            torch.ones(1, 16, dtype=torch.uint8, device=DEV), tables("a", "seqeval"))
    assert float(none) == 0.0


def test_a_group_that_does_not_divide_the_rows_is_refused_before_launch():
    from mtvaf_amd import hip
    t = tables("a", "seqeval")
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=DEV)  # noqa: E731
    pred, gold, mask = z(6, 16, dtype=torch.int32), z(2, 16, dtype=torch.int64), z(2, 16, dtype=torch.uint8)
    out = torch.full((6, 3), -7, dtype=torch.int32, device=DEV)
    tabs = [t[k].data_ptr() for k in ("start", "end", "type_of", "gold_skip")]
    call = lambda R, group: hip.lib().mtvaf_entity_counts_rows(pred.data_ptr(), 16, group, gold.data_ptr(), mask.data_ptr(), *tabs,  # noqa: E731
                                                               R, 16, 11, t["n_types"], out.data_ptr(), None)
    assert call(6, 4) == -1 and call(6, 0) == -1 and call(0, 1) == -1
    torch.cuda.synchronize()
    assert (out == -7).all()
    with pytest.raises(ValueError, match="groups of 4"):
        hip.entity_counts_rows(pred, gold, mask, t["start"], t["end"], t["type_of"], t["gold_skip"], t["n_types"], group=4)
    assert call(6, 3) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
