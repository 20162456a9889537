"""The per-sentence prefix-slot mask of the packed attention launches (mtvaf_prefix_attn_*varlen_*_pm; csrc/attention_args.h,
mask_at<PM>), in all three arithmetics, forward and backward, at the cases of prefix_mask_cases.py:

1. packed rows with pmask against the PADDED launch with the same addmask: the same keys in the same order through the same
   tiles and the same mask values, so every kept row is BIT-identical -- the comparison the project applies between the packed
   and the padded kernels (torch.equal: tests/test_unpad_gpu.py at kernel level, tests/test_ops_gpu.py
   test_varlen_attention_is_the_padded_attention_on_packed_rows);
2. against the float64 restatement, at the tolerances of tests/test_attention_contract_gpu.py (its `compare`);
3. an explicit all-present pmask against pmask = None: the same bits in every output buffer;
4. masked slots: dpk / dpv rows, probabilities and the prefix mass exactly 0.0; a sentence without slots is finite everywhere;
5. dropout live (p = 0.1): as 1 -- the dropout row ids keep the [B, NH, S] indexing in both layouts.

Every float64 comparison prints its figures ("[prefix-mask] ...") before it asserts."""
import gc

import pytest
import torch

import attn_cases as AC
import prefix_mask_cases as PM
from attn_cases import OFFSET, SEED
from test_attention_contract_gpu import Figures, compare, nans

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_ROWS = 37


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    gc.collect()  # (no device epoch word of a dropped captured step may be registered: see test_attention_contract_gpu.py)
    return h


@pytest.fixture(params=["split", "pipe", "bf16"])
def arith(request, hip):
    if request.param == "bf16":
        yield "bf16"
        return
    was = hip.f32_split()
    hip.f32_split(request.param == "split")
    try:
        yield request.param
    finally:
        hip.f32_split(was)


def _outputs(c, M, bf):
    dt = torch.bfloat16 if bf else torch.float32
    o = dict(ctx=nans(M, c.H, dtype=dt), lse=nans(c.B, c.NH, c.S), dqkv=nans(M, 3 * c.H, dtype=dt),
             dpk=nans(c.B, c.NH * c.P * 64), dpv=nans(c.B, c.NH * c.P * 64))
    if bf:
        o["partq"], o["partkv"] = nans(c.B * ((c.S + 63) // 64), c.H), nans(c.B * ((c.T + 63) // 64), 2 * c.H)
    else:
        o["delta"] = nans(c.B, c.NH, c.S)
    return o


def padded(hip, arith, c, p=0.0):
    """The padded launch with the case's [B, P + S] addmask (dctx zero at the padded queries)."""
    bf = arith == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    x = AC.inputs(c, bf16=bf, zero_tail=True)
    qkv, dctx, pk, pv = (x[k].to(DEV).to(dt).contiguous() for k in ("qkv", "dctx", "pk", "pv"))
    am = x["addmask"].to(DEV)
    o = _outputs(c, c.B * c.S, bf)
    a = (c.B, c.S, c.P, c.NH, p, SEED, OFFSET)
    if bf:
        hip.prefix_attn_bf16_fwd(qkv, pk, pv, am, o["ctx"], o["lse"], *a)
        hip.prefix_attn_bf16_bwd(dctx, qkv, pk, pv, am, o["ctx"], o["lse"], o["dqkv"], o["dpk"], o["dpv"], o["partq"], o["partkv"], *a)
    else:
        hip.prefix_attn_fwd(qkv, pk, pv, am, o["ctx"], o["lse"], *a)
        hip.prefix_attn_bwd(dctx, qkv, pk, pv, am, o["ctx"], o["lse"], o["delta"], o["dqkv"], o["dpk"], o["dpv"], *a)
    torch.cuda.synchronize()
    return o


def packed(hip, arith, c, pmask, p=0.0, ordered=True):
    """The packed launch: the kept rows, PAD_ROWS zero rows behind them, the ordered sentence list (longest first: grid slot z is
    not sentence z) or the plain offsets; pmask a device tensor or None."""
    bf = arith == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    x = AC.inputs(c, bf16=bf, zero_tail=True)
    rows = PM.kept_rows(c)
    Mv = len(rows)

    def tok(t):
        out = torch.zeros(Mv + PAD_ROWS, t.shape[1])
        out[:Mv] = t[rows]
        return out.to(DEV).to(dt)
    qkv, dctx = tok(x["qkv"]), tok(x["dctx"])
    pk, pv = x["pk"].to(DEV).to(dt), x["pv"].to(DEV).to(dt)
    cu = (PM.cu_ordered(c) if ordered else PM.cu_plain(c)).to(DEV)
    o = _outputs(c, Mv + PAD_ROWS, bf)
    a = (c.B, c.S, c.P, c.NH, p, SEED, OFFSET)
    if bf:
        hip.prefix_attn_bf16_varlen_fwd_pm(qkv, pk, pv, cu, PAD_ROWS, pmask, o["ctx"], o["lse"], *a)
        hip.prefix_attn_bf16_varlen_bwd_pm(dctx, qkv, pk, pv, cu, PAD_ROWS, pmask, o["ctx"], o["lse"], o["dqkv"], o["dpk"], o["dpv"],
                                           o["partq"], o["partkv"], *a)
    else:
        hip.prefix_attn_varlen_fwd_pm(qkv, pk, pv, cu, PAD_ROWS, pmask, o["ctx"], o["lse"], *a)
        hip.prefix_attn_varlen_bwd_pm(dctx, qkv, pk, pv, cu, PAD_ROWS, pmask, o["ctx"], o["lse"], o["delta"], o["dqkv"], o["dpk"],
                                      o["dpv"], *a)
    torch.cuda.synchronize()
    return o


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_packed_is_padded(c, got, pad):
    rows = PM.kept_rows(c).to(DEV)
    Mv = len(rows)
    live = PM.live_queries(c).to(DEV)
    assert torch.equal(bits(got["ctx"][:Mv]), bits(pad["ctx"][rows])), "context rows"
    assert torch.equal(bits(got["dqkv"][:Mv]), bits(pad["dqkv"][rows])), "dQ | dK | dV rows"
    assert torch.equal(bits(got["lse"][live]), bits(pad["lse"][live])), "lse"
    assert torch.equal(bits(got["dpk"]), bits(pad["dpk"])), "dpk"
    assert torch.equal(bits(got["dpv"]), bits(pad["dpv"])), "dpv"
    if "delta" in got:
        assert torch.equal(bits(got["delta"][live]), bits(pad["delta"][live])), "delta"
    assert float(got["ctx"][Mv:].float().abs().max()) == 0.0 and float(got["dqkv"][Mv:].float().abs().max()) == 0.0, "padding rows"


def assert_finite(c, got):
    """Every element a packed launch writes: lse / delta exist at the kept queries only, everything else is written whole."""
    live = PM.live_queries(c).to(DEV)
    for k, v in got.items():
        v = v[live] if k in ("lse", "delta") else v
        assert bool(torch.isfinite(v.float()).all()), f"{k} holds non-finite values"


# ---------------------------------------------------------------------------------------------------------
# 1. packed with pmask = padded with the same addmask
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PM.CASES, ids=str)
def test_packed_rows_with_a_slot_mask_equal_the_padded_launch(hip, arith, c):
    pm = PM.pmask_of(c).to(DEV)
    got = packed(hip, arith, c, pm)
    assert_packed_is_padded(c, got, padded(hip, arith, c))


# ---------------------------------------------------------------------------------------------------------
# 2. against float64
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PM.CASES, ids=str)
def test_packed_rows_with_a_slot_mask_against_float64(hip, arith, c):
    bf = arith == "bf16"
    got = packed(hip, arith, c, PM.pmask_of(c).to(DEV), ordered=False)
    ref = PM.reference(c, 0.0, bf)
    rows = PM.kept_rows(c)
    Mv = len(rows)
    live = PM.live_queries(c)
    fig = Figures(f"{c.name} {arith}")
    fig.tag = "[prefix-mask] " + fig.tag
    assert_finite(c, got)
    compare(fig, arith, c, "ctx", got["ctx"][:Mv], ref["ctx"][rows])
    compare(fig, arith, c, "dqkv", got["dqkv"][:Mv], ref["dqkv"][rows])
    compare(fig, arith, c, "dpk", got["dpk"], ref["dpk"])
    compare(fig, arith, c, "dpv", got["dpv"], ref["dpv"])
    compare(fig, arith, c, "lse", got["lse"].cpu()[live], ref["lse"][live])
    if not bf:
        compare(fig, arith, c, "delta", got["delta"].cpu()[live], ref["delta"][live])
    fig.settle()


# ---------------------------------------------------------------------------------------------------------
# 3. an all-present mask given explicitly = no mask
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("P,S", PM.SHAPES)
def test_an_all_present_mask_is_no_mask(hip, arith, P, S, p):
    c = PM.case(P, S, "none")
    none = packed(hip, arith, c, None, p=p)
    zeros = packed(hip, arith, c, torch.zeros(c.B, c.P, device=DEV), p=p)
    assert set(none) == set(zeros)
    rows = PM.kept_rows(c)
    live = PM.live_queries(c).to(DEV)
    for k in none:
        a, b = none[k], zeros[k]
        if k in ("lse", "delta"):  # (written at the kept queries only)
            a, b = a[live], b[live]
        assert torch.equal(bits(a), bits(b)), k
    assert bool(torch.isfinite(none["ctx"].float()).all()) and len(rows) == sum(c.lengths)


# ---------------------------------------------------------------------------------------------------------
# 4. exact zeros at masked slots; a sentence without slots
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in PM.CASES if not c.name.endswith("none")], ids=str)
def test_masked_slots_get_exact_zeros(hip, arith, c):
    bf = arith == "bf16"
    got = packed(hip, arith, c, PM.pmask_of(c).to(DEV), p=0.1)
    m = PM.slot_masked(c)
    mh = m[:, None, :].expand(c.B, c.NH, c.P).to(DEV)
    for k in ("dpk", "dpv"):
        g = got[k].view(c.B, c.NH, c.P, 64)
        assert float(g[mh].abs().max()) == 0.0, k
        assert float(g[~mh].abs().max()) > 0.0 or not bool((~mh).any()), k
    assert_finite(c, got)
    if bf:
        return
    # the probabilities on request (padded layout: its addmask carries the prefix columns) and the prefix mass
    x = AC.inputs(c)
    probs, mass = nans(c.B, c.NH, c.S, c.T), nans(c.B, c.NH, c.S)
    hip.prefix_attn_probs(x["qkv"].to(DEV), x["pk"].to(DEV), x["addmask"].to(DEV), probs, mass, c.B, c.S, c.P, c.NH)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(mass).all())
    sel = m[:, None, None, :].expand(c.B, c.NH, c.S, c.P).to(DEV)
    assert float(probs[..., :c.P][sel].abs().max()) == 0.0
    if c.name.endswith("one_full"):
        assert float(mass[PM.FULL].abs().max()) == 0.0  # no slot left: the whole mass is the masked slots' share
        assert float(mass[0].min()) > 0.0
    # (the mass is an fp32 sum of P probabilities <= 1: P roundings of at most 2^-24 each)
    want = probs[..., :c.P].double().sum(-1)
    assert float((mass.double() - want).abs().max()) <= c.P * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------
# 5. dropout live
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in PM.CASES if c.name.endswith(("holes", "one_full"))], ids=str)
def test_packed_rows_with_a_slot_mask_and_dropout_equal_the_padded_launch(hip, arith, c):
    got = packed(hip, arith, c, PM.pmask_of(c).to(DEV), p=0.1)
    pad = padded(hip, arith, c, p=0.1)
    assert_packed_is_padded(c, got, pad)
    plain = packed(hip, arith, c, PM.pmask_of(c).to(DEV))
    live = PM.live_queries(c).to(DEV)
    assert torch.equal(got["lse"][live], plain["lse"][live])  # (lse is that of the undropped scores)
    assert not torch.equal(bits(got["ctx"]), bits(plain["ctx"]))  # (dropout was live)
