"""Entity counting on the MI355X: `mtvaf_entity_counts` / `EntityScorer` against the sequential restatement of its rule
(tests/entity_cases.py) and against the reference-made counts of tests/golden/entity_chunks.npz -- every comparison is exact
integer equality of the whole counter -- and `TVNetSAModel2` with ``args.score_entities``."""
import types

import numpy as np
import pytest
import torch
from transformers import BertConfig

import entity_cases as E
import params as P
from test_entity_counts import fixture, fixture_counter

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCHEMES = ("seqeval", "reference")
SETS = ("a", "b", "c")
SIZES_S = (1, 2, 63, 64, 65, 128, 130, 512)
SIZES_B = (1, 3, 37)


def scorer(s, scheme):
    from mtvaf_amd.metrics import EntityScorer
    return EntityScorer(E.label_map(s), scheme=scheme, device=DEV)


def run(sc, gold, pred, mask):
    """one update from a zeroed counter -> the counter as a numpy array"""
    sc.reset()
    sc.update(torch.from_numpy(pred).to(DEV), torch.from_numpy(gold).to(DEV), torch.from_numpy(mask).to(DEV))
    return sc.counts.cpu().numpy()


def check(sc, s, scheme, gold, pred, mask, what):
    want = E.counter(sc.types, E.restate(E.label_map(s), scheme, gold, pred, mask))
    got = run(sc, gold, pred, mask)
    assert got.tolist() == want.tolist(), what
    return want


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("s", SETS)
def test_every_size_against_the_restatement(s, scheme):
    """S in {1, 2, 63, 64, 65, 128, 130, 512} x B in {1, 3, 37}; the mask kind, the prediction mix and the gold-skip density rotate
    through the shapes (each is crossed with the others at one shape below)."""
    sc, lmap, rng = scorer(s, scheme), E.label_map(s), np.random.default_rng(7)
    k, chunks_seen = 0, 0
    for S in SIZES_S:
        for B in SIZES_B:
            mk, pk, dens = E.MASKS[k % 5], E.PREDS[(k // 2) % 4], (0.0, 0.3)[k % 2]
            gold, pred, mask = E.make_case(rng, lmap, B, S, mk, pk, dens)
            want = check(sc, s, scheme, gold, pred, mask, (S, B, mk, pk, dens))
            chunks_seen += int(want[:-2].sum())
            k += 1
    assert chunks_seen > 5000  # the cases are not empty


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("s", SETS)
def test_masks_predictions_and_skip_densities_crossed(s, scheme):
    """full / ragged / hole / all-zero row / only column 0  x  pred = gold / uniform / half agreeing / with -1 and ids >= C (on both
    sides)  x  gold-skip density 0 / 0.3, at S = 130 (three 64-bit words, the last one partial), B = 5."""
    sc, lmap, rng = scorer(s, scheme), E.label_map(s), np.random.default_rng(11)
    for mk in E.MASKS:
        for pk in E.PREDS:
            for dens in (0.0, 0.3):
                gold, pred, mask = E.make_case(rng, lmap, 5, 130, mk, pk, dens)
                want = check(sc, s, scheme, gold, pred, mask, (mk, pk, dens))
                if pk == "equal" and mk != "col0":
                    assert (want[0:-2:3] == want[1:-2:3]).all() and want[-2] == want[-1] > 0
                    if scheme == "reference":  # no unopened chunks there: every chunk is correct
                        assert (want[0:-2:3] == want[2:-2:3]).all()
                if mk == "col0":
                    assert not want.any()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("s", SETS)
def test_long_skipped_runs_and_word_boundaries(s, scheme):
    """>= 70 skipped columns inside one entity (the previous / next kept column lies more than one 64-bit word away), an entity
    across columns 63 | 64, one that ends at 63 on the gold side and at 64 on the predicted side; then the same with every column
    up to the last one kept (S = 256 and S = 512)."""
    sc, lmap = scorer(s, scheme), E.label_map(s)
    for S in (256, 512):
        gold, pred, mask = E.long_skip_case(lmap, S)
        want = check(sc, s, scheme, gold, pred, mask, S)
        per, _, kept = E.restate(lmap, scheme, gold, pred, mask)
        ty = [n for n, _ in E.labels_of(lmap) if n[:2] == "B-"][0][2:]  # the type the case builds its entities of
        assert per[ty] == [6, 5, 3] and kept == 3 * (S - 1) - 79 - 74, per  # predicted, gold, correct: worked out by hand
        assert want[-1] == kept


def test_updates_accumulate_reset_zeroes_and_runs_repeat():
    sc, lmap, rng = scorer("a", "seqeval"), E.label_map("a"), np.random.default_rng(3)
    one = E.make_case(rng, lmap, 37, 65, "ragged", "mixed", 0.3)
    two = E.make_case(rng, lmap, 9, 128, "hole", "wild", 0.3)
    c1, c2 = run(sc, *one), run(sc, *two)
    assert c1.any() and c2.any()
    assert run(sc, *one).tolist() == c1.tolist(), "two runs of the same input differ"
    sc.reset()
    assert not sc.counts.cpu().numpy().any()
    for gold, pred, mask in (one, two):
        sc.update(torch.from_numpy(pred).to(DEV), torch.from_numpy(gold).to(DEV), torch.from_numpy(mask).to(DEV))
    assert sc.counts.cpu().numpy().tolist() == (c1 + c2).tolist()
    got = sc.compute()
    t = sc.types.index("POS")
    assert got["POS"]["predicted"] == int((c1 + c2)[3 * t]) and got["micro"]["correct"] == int((c1 + c2)[2:-2:3].sum())
    sc.reset()
    assert not sc.counts.cpu().numpy().any()


def test_tags_wider_than_the_labels_and_other_mask_dtypes():
    """pred is read with its own row stride ([B, S + 1] as the packed tags | length tensor, or a column slice of it); an int64
    attention mask is cast."""
    sc, lmap, rng = scorer("a", "reference"), E.label_map("a"), np.random.default_rng(5)
    gold, pred, mask = E.make_case(rng, lmap, 6, 65, "ragged", "mixed", 0.3)
    want = E.counter(sc.types, E.restate(lmap, "reference", gold, pred, mask)).tolist()
    packed = torch.from_numpy(np.concatenate([pred, mask.sum(1, keepdims=True).astype(np.int32)], 1)).to(DEV)
    for tags in (packed, packed[:, :65]):
        sc.reset()
        sc.update(tags, torch.from_numpy(gold).to(DEV), torch.from_numpy(mask.astype(np.int64)).to(DEV))
        assert sc.counts.cpu().numpy().tolist() == want


def test_shapes_beyond_the_limits_are_errors():
    from mtvaf_amd import hip
    from mtvaf_amd.metrics import EntityScorer
    sc = scorer("a", "seqeval")
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="S=513"):
        sc.update(z(2, 513, dtype=torch.int32), z(2, 513, dtype=torch.int64), z(2, 513, dtype=torch.uint8))
    assert not sc.counts.cpu().numpy().any()
    with pytest.raises(ValueError, match="64"):
        EntityScorer({**E.label_map("c"), "B-EXTRA": 64}, device=DEV)
    tabs = [z(66 * 66, dtype=torch.uint8), z(66 * 66, dtype=torch.uint8), z(66, dtype=torch.int32), z(65, dtype=torch.uint8)]
    batch = [z(2, 16, dtype=torch.int32), z(2, 16, dtype=torch.int64), z(2, 16, dtype=torch.uint8)]
    args = [batch[0].data_ptr(), 16, batch[1].data_ptr(), batch[2].data_ptr(), *[t.data_ptr() for t in tabs]]
    cnt = z(14, dtype=torch.int64)
    assert hip.lib().mtvaf_entity_counts(*args, 2, 16, 65, 4, cnt.data_ptr(), None) == -1   # C = 65
    assert hip.lib().mtvaf_entity_counts(*args[:1], 513, *args[2:], 2, 513, 11, 4, cnt.data_ptr(), None) == -1  # S = 513
    torch.cuda.synchronize()
    assert not cnt.cpu().numpy().any()


@pytest.mark.parametrize("s", ["a", "b"])
def test_kernel_equals_the_reference_counts_of_the_fixture(s):
    fx = fixture()
    sc = scorer(s, "reference")
    got = run(sc, fx[f"{s}_gold"], fx[f"{s}_pred"], fx[f"{s}_mask"])
    assert got.tolist() == fixture_counter(fx, s, sc.types).tolist()


# ---- the model ---------------------------------------------------------------------------------------------------------------
LABELS = E.SET_A
LABEL_MAP = {label: i for i, label in enumerate(LABELS, 1)}


def tiny_model(**kw):
    from mtvaf_amd.models.bert_model import TVNetSAModel2
    cfg = P.EncCfg(vocab_size=500, hidden=128, heads=2, inter=256, layers=2, max_pos=64)
    args = types.SimpleNamespace(bert_name="bert-base-uncased", use_prefix=False, vao=False, noauxloss=True, use_probe=False,
                                 n_gpu=1, alpha=0.5, beta=0.0, prefix_len=4, prefix_dim=768, device=DEV, resnet_root=None,
                                 use_152=False, **kw)
    args.bert_config = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                                  num_attention_heads=cfg.heads, intermediate_size=cfg.inter,
                                  max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.eps,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu", pad_token_id=0)
    torch.manual_seed(0)
    return cfg, TVNetSAModel2(LABELS, None, args).to(DEV).eval()


@pytest.mark.parametrize("B", [16, 32])  # 32 x 32 tokens: the Viterbi launch (and the count behind it) runs on the second stream
@pytest.mark.parametrize("flag", [True, "reference"])
def test_model_scores_its_own_tags(flag, B):
    from mtvaf_amd.metrics import label_sequences
    scheme = "seqeval" if flag is True else flag
    cfg, plain = tiny_model()
    _, scored = tiny_model(score_entities=flag)
    assert plain.entity_scorer is None
    assert scored.entity_scorer is not None and scored.entity_scorer.scheme == scheme
    scored.load_state_dict(plain.state_dict())
    y_true, y_pred = [], []
    for step in range(2):
        ids, mask, tt, labels = (t.to(DEV) for t in P.text_batch(cfg, 40 + step, B, 32, lo_id=5))
        labels[:, 0] = LABEL_MAP["[CLS]"]
        a = plain(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
        b = scored(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels)
        assert float(a.loss) == float(b.loss) and list(a.logits) == list(b.logits)
        assert b.logits.device_tags.dtype == torch.int32 and tuple(b.logits.device_tags.shape) == (B, 32)
        t, p = label_sequences(labels, mask, b.logits, LABEL_MAP)
        y_true += t
        y_pred += p
    sc = scored.entity_scorer
    as_labels = lambda rows: [[(n, n == "O") for n in row] for row in rows]  # noqa: E731
    want = E.counter(sc.types, E.count_sequences(scheme, as_labels(y_true), as_labels(y_pred)))
    assert sc.counts.cpu().numpy().tolist() == want.tolist()
    assert want[-1] > 0 and want[:-2].any()
    got = sc.compute()
    assert got["token_accuracy"] == want[-2] / want[-1]
    assert got["micro"]["predicted"] == int(want[0:-2:3].sum()) and got["micro"]["support"] == int(want[1:-2:3].sum())
    # a forward without labels counts nothing
    before = sc.counts.clone()
    scored(input_ids=ids, attention_mask=mask, token_type_ids=tt)
    assert torch.equal(sc.counts, before)
