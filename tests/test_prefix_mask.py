"""The yardstick of the prefix-slot mask tests, on the CPU: the float64 restatement (prefix_mask_cases.reference) has the
properties the GPU tests hold the kernels to -- a masked slot's probability is effectively 0, no gradient reaches it, and a
sentence that lost every slot is the P = 0 sentence -- and the new C entries are declared, bound and refuse a mask whose extent
cannot be right (host-side checks: no GPU call)."""
import ctypes

import pytest
import torch

import abi_header
import attn_cases as AC
import prefix_mask_cases as PM

NEW_ENTRIES = ["mtvaf_prefix_attn_varlen_fwd_pm", "mtvaf_prefix_attn_varlen_bwd_pm", "mtvaf_prefix_attn_bf16_varlen_fwd_pm",
               "mtvaf_prefix_attn_bf16_varlen_bwd_pm", "mtvaf_kl_logsoftmax_masked_fwd", "mtvaf_kl_logsoftmax_masked_bwd"]


def test_cases_are_what_their_names_state():
    assert len(PM.CASES) == len(PM.SHAPES) * len(PM.PATTERNS) == 16
    for c in PM.CASES:
        assert (c.B, c.NH, c.H) == (3, 2, 128) and set(c.lengths) == {c.S, 5, 1}
        order = PM.cu_ordered(c)[c.B + 1:].tolist()
        assert order == [1, 0, 2] and order != list(range(c.B))  # longest first is not the batch order
        m = PM.slot_masked(c)
        pm = PM.pmask_of(c)
        assert pm.shape == (c.B, c.P) and pm.dtype == torch.float32
        assert torch.equal(pm, AC.inputs(c)["addmask"][:, :c.P])  # the prefix columns of the padded layout's mask
        assert set(pm.unique().tolist()) <= {0.0, -10000.0}
        pat = c.name.rsplit("_", 1)[-1]
        if c.name.endswith("none"):
            assert not bool(m.any())
        elif c.name.endswith("one_full"):
            assert bool(m[PM.FULL].all()) and int(m.sum()) == c.P and c.lengths[PM.FULL] == 1
        elif pat == "last":
            assert bool(m[:, -1].all()) and int(m.sum()) == c.B
        else:
            rows = [tuple(m[b].tolist()) for b in range(c.B)]
            assert len(set(rows)) == c.B and all(0 < sum(r) for r in rows) and not bool(m[2, -1])
    assert any(c.P > AC.KT for c in PM.CASES) and any(c.P + c.S <= AC.KT for c in PM.CASES)
    assert any(c.P < AC.KT < c.P + c.S for c in PM.CASES)


@pytest.mark.parametrize("c", [c for c in PM.CASES if not c.name.endswith("none")], ids=str)
def test_masked_slots_have_no_probability_and_no_gradient(c):
    ref = PM.reference(c)
    m = PM.slot_masked(c)
    live = PM.live_queries(c)
    probs = ref["probs"][:, :, :, :c.P]                                  # [B,NH,S,P]
    sel = live[..., None] & m[:, None, None, :]
    assert bool(sel.any()) and float(probs[sel].max()) < 1e-300
    dpk, dpv = (ref[k].view(c.B, c.NH, c.P, AC.D) for k in ("dpk", "dpv"))
    mh = m[:, None, :].expand(c.B, c.NH, c.P)
    assert float(dpk[mh].abs().max()) == 0.0 and float(dpv[mh].abs().max()) == 0.0
    assert float(dpk[~mh].abs().min()) > 0.0 or not bool((~mh).any())   # (... and the live slots do get one)
    for k in ("ctx", "lse", "dqkv", "dpk", "dpv", "delta"):
        assert bool(torch.isfinite(ref[k]).all()), k


@pytest.mark.parametrize("c", [c for c in PM.CASES if c.name.endswith("one_full")], ids=str)
def test_a_sentence_without_slots_is_the_sentence_without_a_prefix(c):
    """Sentence FULL of the one_full pattern against the attention over its text keys alone, written out in float64."""
    b, n = PM.FULL, c.lengths[PM.FULL]
    x = AC.inputs(c, zero_tail=True)
    ref = PM.reference(c)
    qkv = x["qkv"].double().view(c.B, c.S, 3, c.NH, AC.D)[b, :n].clone().requires_grad_(True)
    q, k, v = (qkv[:, i].permute(1, 0, 2) for i in range(3))             # [NH,n,D]
    s = q @ k.transpose(-1, -2) * AC.SCALE
    lse = torch.logsumexp(s, -1)
    ctx = (torch.exp(s - lse[..., None]) @ v).permute(1, 0, 2).reshape(n, c.H)
    (ctx * x["dctx"].double().view(c.B, c.S, c.H)[b, :n]).sum().backward()
    tol = dict(rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref["ctx"].view(c.B, c.S, c.H)[b, :n], ctx.detach(), **tol)
    assert torch.allclose(ref["lse"][b, :, :n], lse.detach(), **tol)
    assert torch.allclose(ref["dqkv"].view(c.B, c.S, 3, c.NH, AC.D)[b, :n], qkv.grad, **tol)
    assert float(ref["dpk"][b].abs().max()) == 0.0 and float(ref["dpv"][b].abs().max()) == 0.0


def test_new_entries_are_declared_and_bound():
    from mtvaf_amd import hip
    declared = {name for _, name, _ in abi_header.prototypes()}
    for n in NEW_ENTRIES:
        assert n in declared and n in hip._SIGS, n
        assert (hip._SIGS[n][0], list(hip._SIGS[n][1])) == abi_header.signature(n), n
        assert "pmask" in abi_header.comment_before("mtvaf_prefix_attn_varlen_fwd_pm")
    assert ("pmask", "const float*") in abi_header.structs()["mtvaf_layer_t"]
    for w in ("prefix_attn_varlen_fwd_pm", "prefix_attn_varlen_bwd_pm", "prefix_attn_bf16_varlen_fwd_pm",
              "prefix_attn_bf16_varlen_bwd_pm"):
        assert callable(getattr(hip, w)), w


def test_new_entries_refuse_a_mask_of_the_wrong_extent():
    """pmask with P == 0, and P > 0 with pmask_len != B * P: MTVAF_ERR_ARG from the host-side checks, before any launch (the
    pointers are never dereferenced: no GPU is needed)."""
    from mtvaf_amd import hip
    L = hip.lib()
    ERR_ARG = abi_header.defines()["MTVAF_ERR_ARG"]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # a non-NULL stand-in for every pointer
    Bn, S, NHn = 3, 16, 2

    def fwd32(pm, n, P):
        return L.mtvaf_prefix_attn_varlen_fwd_pm(p, p, p, p, 0, pm, n, p, p, Bn, S, P, NHn, 64, 0.0, 0, 0, None, 0, None)

    def bwd32(pm, n, P):
        return L.mtvaf_prefix_attn_varlen_bwd_pm(p, p, p, p, p, 0, pm, n, p, p, p, p, p, p, Bn, S, P, NHn, 64, 0.0, 0, 0, None, 0, None)

    def fwd16(pm, n, P):
        return L.mtvaf_prefix_attn_bf16_varlen_fwd_pm(p, p, p, p, 0, pm, n, p, p, Bn, S, P, NHn, 64, 0.0, 0, 0, None)

    def bwd16(pm, n, P):
        return L.mtvaf_prefix_attn_bf16_varlen_bwd_pm(p, p, p, p, p, 0, pm, n, p, p, p, p, p, p, p, Bn, S, P, NHn, 64, 0.0, 0, 0, None)

    for f in (fwd32, bwd32, fwd16, bwd16):
        assert f(p, 0, 0) == ERR_ARG, f.__name__           # a mask without a prefix
        assert f(p, Bn * 4, 0) == ERR_ARG, f.__name__
        assert f(p, Bn * 4 - 1, 4) == ERR_ARG, f.__name__   # P > 0, wrong extent
        assert f(p, 4, 4) == ERR_ARG, f.__name__            # (one sentence's worth)
        assert f(p, Bn * 5, 4) == ERR_ARG, f.__name__
    # the masked image-tag loss wants its row mask
    assert L.mtvaf_kl_logsoftmax_masked_fwd(p, p, None, p, p, Bn, 8, None) == ERR_ARG
    assert L.mtvaf_kl_logsoftmax_masked_bwd(p, 1.0, p, p, None, p, Bn, 8, None) == ERR_ARG
