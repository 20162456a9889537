"""Per-sentence CRF likelihoods and tag marginals on the CPU: every case test_crf_llh_gpu.py runs goes through the
float32 and float64 oracle here, so the acceptance rule of crf_llh_cases is known to be well-formed and the references to
be what they claim (probabilities, brute-force answers) before a kernel is measured against them; plus the parts of the
public surface that need no GPU (reduction validation, the model's switches)."""
import types

import pytest
import torch
from transformers import BertConfig

import crf_llh_cases as L
from oracle import mtvaf_oracle as O


@pytest.mark.parametrize("case", L.CASES, ids=str)
def test_acceptance_rule_is_well_formed_and_met_by_the_float32_reference(case):
    ref = L.reference(case)
    for name in L.QUANTITIES:
        b = ref.bound[name]
        assert b == b and 0.0 < b < float("inf"), (name, b)
        assert L.ratio(name, ref.r32[name], ref.r64[name], b) <= 0.25 + 1e-12, name  # (the rule's factor 4)


@pytest.mark.parametrize("case", L.CASES, ids=str)
def test_reference_marginals_are_probabilities(case):
    ref = L.reference(case)
    em, tags, mask, *_ = ref.inputs
    marg, on = ref.r64["marg"], mask.bool()
    on[:, 0] = True
    assert bool((marg[~on] == 0).all())
    assert float(marg.min()) >= -1e-12
    assert float((marg.sum(-1)[on] - 1).abs().max()) <= 1e-10
    # weight 0 gives exact zeros, and the emission gradient of llh is one-hot(gold) - marginal at every step that counts
    w = ref.w
    onehot = torch.nn.functional.one_hot(tags, em.shape[2]).double() * on[..., None]
    assert float((ref.r64["dem"] - w.double()[:, None, None] * (onehot - marg)).abs().max()) <= 1e-10
    if len(w) >= 2:
        assert float(w[1]) == 0.0 and bool((ref.r64["dem"][1] == 0).all())
        assert bool((w > 0).any()) and (len(w) < 3 or bool((w < 0).any()))


@pytest.mark.parametrize("case", L.BRUTE, ids=str)
def test_reference_equals_the_bruteforce_answers(case):
    ref = L.brute_reference(case)
    for name in ("llh", "logz", "marg"):
        assert float((ref.r64[name] - ref.brute[name]).abs().max()) <= 1e-10, name
    if case[2] ** max(case[4]) <= 1000:  # the oracle's own enumeration (a Python loop over the paths) where it is quick
        em, _, mask, start, end, trans = ref.inputs
        logz, _ = O.crf_bruteforce(em, mask, start, end, trans)
        assert float((ref.brute["logz"] - torch.tensor(logz, dtype=torch.float64)).abs().max()) <= 1e-10


def test_case_lists_cover_the_kernels_branch_points():
    narrow = [c for c in L.NARROW if c[3] == 1]
    assert {c[2] for c in narrow} == {1, 2, 11, 16} and {c[1] for c in narrow} == {1, 2, 16, 17, 65}
    assert {c[0] for c in narrow} == {1, 3, 70} and len(narrow) == 60
    assert any(c[3] < 0 for c in L.NARROW) and any(c[3] > 1 for c in L.NARROW)
    assert L.WIDE == [(4, 5, 17, 1), (2, 1, 64, 1), (4, 66, 48, -1), (6, 128, 64, 6), (3, 512, 64, 1)]
    holes = L.reference((3, 65, 11, -1)).inputs[2]
    assert any(int(row[: int(row.nonzero().max()) + 1].sum()) < int(row.nonzero().max()) + 1 for row in holes)


def test_invalid_reduction_raises_value_error_before_any_kernel():
    from mtvaf_amd.modules.crf import CRF
    crf = CRF(5, batch_first=True)
    em, tags = torch.zeros(2, 3, 5), torch.zeros(2, 3, dtype=torch.long)
    for bad in ("batch_mean", "", "Mean", None):
        with pytest.raises(ValueError, match="invalid reduction"):
            crf(em, tags, reduction=bad)
    assert CRF.REDUCTIONS == ("none", "sum", "mean", "token_mean")


def _args(**kw):
    cfg = BertConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    return types.SimpleNamespace(bert_name="bert-base-uncased", bert_config=cfg, use_prefix=False, vao=False,
                                 noauxloss=True, use_probe=False, n_gpu=1, alpha=0.0, prefix_len=4, prefix_dim=768,
                                 device="cpu", resnet_root=None, use_152=False, **kw)


def test_model_switches_default_to_todays_behaviour():
    """A reference ``args`` namespace has neither switch: the loss is the batch-mean NLL and no marginals are made."""
    from mtvaf_amd.models import bert_model as M
    args = _args()
    assert not hasattr(args, "crf_reduction") and not hasattr(args, "output_tag_marginals")
    assert M._crf_reduction(args) == "mean" and not M._arg(args, "output_tag_marginals")
    m = M.TVNetSAModel2(["O", "B", "I"], None, args)
    assert m.last_tag_marginals is None
    for r in ("mean", "token_mean", "sum"):
        assert M._crf_reduction(_args(crf_reduction=r)) == r
    assert M._arg(_args(output_tag_marginals=True), "output_tag_marginals") is True
    with pytest.raises(ValueError, match="crf_reduction"):
        M.TVNetSAModel2(["O", "B", "I"], None, _args(crf_reduction="none"))
