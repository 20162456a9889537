"""The prefix-attention kernels of csrc/attention_skeleton.h against a float64 reference, in all three arithmetics (split bf16
products = the fp32 default, the fp32 MFMA pipe, bf16 operands), at the cases of attn_cases.py: forward and backward, lse and
delta, the zero-tail variants, dropout live with the mask replicated on the host, and the packed layout with the plain and the
ordered sentence list -- each directly against float64, never one kernel variant against another.

Tolerances are the project's own (tests/test_ops_gpu.py): fp32 `close` at rtol 2e-4 for the context, 5e-4 for gradients and
delta, 1e-5 for lse; bf16 norm-relative 6e-3 forward and 1.2e-2 gradients.  The element-wise `close` at rtol 2e-2 on bf16
quantities is this file's own addition (a norm hides a single wrong row); it is the bound test_ops_gpu.py uses for bf16 `close`.
Only the bf16 gradients of the two steep cases get more: attn_cases.BF16_GRAD, 4 x the error against float64 of the same
formula in fp32 torch with P rounded to bf16 before P V, recomputed and held by test_attn_cases.py.  The fp32 evaluation of
every case, steep ones included, stays below 1.1e-5 in the `close` measure (bounds 2e-4 / 5e-4), so no fp32 bound is widened.

Every test prints its figures ("[attn-contract] ...": the smallest rtol / the norm-relative error that would have passed)
before it asserts."""
import functools
import gc

import pytest
import torch

import attn_cases as AC
from attn_cases import BF16_GRAD, BY_NAME, CASES, OFFSET, SEED, need, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    # keep_mask replicates host-fed masks: no device epoch word may be registered while these tests run.  A captured step
    # (mtvaf_amd.graph) registers one and unregisters it when it is closed or collected; collect what earlier modules dropped,
    # and leave a word that a LIVE step still owns alone: every dropout test below then fails on the mask, loudly, instead of
    # that step silently losing its epoch.
    gc.collect()
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


@functools.lru_cache(maxsize=None)
def keep_of(name, p):
    c = BY_NAME[name]
    return AC.keep_mask(SEED, OFFSET, c.B, c.NH, c.S, c.T, p)


@functools.lru_cache(maxsize=None)
def ref_of(name, p, bf16, zero_tail):
    """The float64 reference of a case, computed once and shared (nobody writes into it)."""
    c = BY_NAME[name]
    return AC.reference(c, keep=keep_of(name, p) if p else None, p=p, bf16=bf16, zero_tail=zero_tail)


# ---------------------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------------------
class Figures:
    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, what, value, bound):
        self.rows.append((what, value, bound))

    def settle(self):
        print(f"[attn-contract] {self.tag}: " + "  ".join(f"{w} {v:.2e}/{b:.1e}" for w, v, b in self.rows))
        bad = [(w, v, b) for w, v, b in self.rows if not v <= b]
        assert not bad, f"{self.tag}: " + ", ".join(f"{w} {v:.3e} > {b:.1e}" for w, v, b in bad)


# ---------------------------------------------------------------------------------------------------------
# launches: every output buffer is NaN before the kernel runs
# ---------------------------------------------------------------------------------------------------------
def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def launch(hip, arith, c, x, p=0.0, zero_tail=False, cu=None, rows=None, pad_rows=0):
    """Forward + backward of case c on inputs x, padded (cu None) or packed (cu, rows = kept_rows, pad_rows zero rows behind).
    -> dict of device tensors."""
    B, S, P, NH, H, T = c.B, c.S, c.P, c.NH, c.H, c.T
    bf = arith == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    M = B * S if cu is None else len(rows) + pad_rows

    def tok(t):  # token rows of the launch's layout
        if cu is None:
            return t.to(DEV).to(dt).contiguous()
        out = torch.zeros(M, t.shape[1])
        out[:len(rows)] = t[rows]
        return out.to(DEV).to(dt)
    qkv, dctx = tok(x["qkv"]), tok(x["dctx"])
    pk, pv = (x["pk"].to(DEV).to(dt), x["pv"].to(DEV).to(dt)) if P else (None, None)
    am = x["addmask"].to(DEV)
    o = dict(ctx=nans(M, H, dtype=dt), lse=nans(B, NH, S), dqkv=nans(M, 3 * H, dtype=dt),
             dpk=nans(B, NH * P * 64) if P else None, dpv=nans(B, NH * P * 64) if P else None)
    if bf:
        o["partq"], o["partkv"] = nans(B * ((S + 63) // 64), H), nans(B * ((T + 63) // 64), 2 * H)
    else:
        o["delta"] = nans(B, NH, S)
    if cu is None:
        if bf:
            hip.prefix_attn_bf16_fwd(qkv, pk, pv, am, o["ctx"], o["lse"], B, S, P, NH, p, SEED, OFFSET)
            hip.prefix_attn_bf16_bwd(dctx, qkv, pk, pv, am, o["ctx"], o["lse"], o["dqkv"], o["dpk"], o["dpv"], o["partq"], o["partkv"],
                                     B, S, P, NH, p, SEED, OFFSET, zero_tail=zero_tail)
        else:
            hip.prefix_attn_fwd(qkv, pk, pv, am, o["ctx"], o["lse"], B, S, P, NH, p, SEED, OFFSET)
            hip.prefix_attn_bwd(dctx, qkv, pk, pv, am, o["ctx"], o["lse"], o["delta"], o["dqkv"], o["dpk"], o["dpv"], B, S, P, NH,
                                p, SEED, OFFSET, zero_tail=zero_tail)
    else:
        cud = cu.to(DEV)
        if bf:
            hip.prefix_attn_bf16_varlen_fwd(qkv, pk, pv, cud, pad_rows, o["ctx"], o["lse"], B, S, P, NH, p, SEED, OFFSET)
            hip.prefix_attn_bf16_varlen_bwd(dctx, qkv, pk, pv, cud, pad_rows, o["ctx"], o["lse"], o["dqkv"], o["dpk"], o["dpv"],
                                            o["partq"], o["partkv"], B, S, P, NH, p, SEED, OFFSET)
        else:
            hip.prefix_attn_varlen_fwd(qkv, pk, pv, cud, pad_rows, o["ctx"], o["lse"], B, S, P, NH, p, SEED, OFFSET)
            hip.prefix_attn_varlen_bwd(dctx, qkv, pk, pv, cud, pad_rows, o["ctx"], o["lse"], o["delta"], o["dqkv"], o["dpk"], o["dpv"],
                                       B, S, P, NH, p, SEED, OFFSET)
    torch.cuda.synchronize()
    return {k: v for k, v in o.items() if v is not None}


def compare(fig, arith, c, what, got, ref):
    """One quantity at the tolerance of its arithmetic."""
    bf = arith == "bf16"
    if what == "lse":
        fig.add("lse", need(got, ref), 1e-5)
    elif what == "ctx":
        if bf:
            fig.add("ctx(norm)", relerr(got, ref), 6e-3)
            fig.add("ctx", need(got, ref), 2e-2)
        else:
            fig.add("ctx", need(got, ref), 2e-4)
    elif bf:
        nb, eb = BF16_GRAD.get(c.name, (1.2e-2, 2e-2))
        fig.add(what + "(norm)", relerr(got, ref), nb)
        fig.add(what, need(got, ref), eb)
    else:
        fig.add(what, need(got, ref), 5e-4)


def check_padded(fig, arith, c, got, ref):
    """Outputs of a padded launch against the float64 reference: every row of every sentence but the exempt ones."""
    B, S, P, NH, H, T = c.B, c.S, c.P, c.NH, c.H, c.T
    for k, v in got.items():  # every element was written, and nothing is NaN or infinite even in an exempt sentence
        assert bool(torch.isfinite(v.float()).all()), f"{fig.tag}: {k} holds non-finite values"
    live = [b for b in range(B) if b not in c.exempt]
    sent = lambda t: t.reshape(B, -1)[live]
    for k in ("ctx", "lse", "delta", "dqkv", "dpk", "dpv"):
        if k in got:
            compare(fig, arith, c, k, sent(got[k]), sent(ref[k]))
    # gradient rows of masked text keys (trailing padding and holes alike): exact zeros
    dead = (AC.mask_of(c)[:, P:] == 0)
    for b in c.exempt:
        dead[b] = False
    kv = got["dqkv"].float().cpu().view(B, S, 3, H)[:, :, 1:]
    assert bool(dead.any()) and float(kv[dead].abs().max()) == 0.0, f"{fig.tag}: dK | dV of masked text keys"
    assert float(ref["dqkv"].view(B, S, 3, H)[:, :, 1:][dead].abs().max()) == 0.0
    if arith == "bf16":  # per-block column sums: against the reference gradient and against the stored one
        nqt, nkt = (S + 63) // 64, (T + 63) // 64
        pq = got["partq"].view(B, nqt, H)[live].sum((0, 1)).double().cpu()
        pkv = got["partkv"].view(B, nkt, 2 * H)[live].sum((0, 1)).double().cpu()
        want = ref["dqkv"].view(B, S, 3 * H)[live].sum((0, 1))
        stored = got["dqkv"].double().cpu().view(B, S, 3 * H)[live].sum((0, 1))
        nb, eb = BF16_GRAD.get(c.name, (1.2e-2, 2e-2))
        fig.add("partials(norm)", relerr(torch.cat([pq, pkv]), want), nb)
        fig.add("partials-vs-stored", need(torch.cat([pq, pkv]), stored), 2e-2)
    for b in c.exempt:  # every score carries -10000 there: fp32 keeps 2^-10 of a log2 unit at 14427, ~1e-3 on a probability
        fig.add(f"ctx[exempt {b}]", need(got["ctx"].view(B, S, H)[b], ref["ctx"].view(B, S, H)[b]), 5e-3)


# ---------------------------------------------------------------------------------------------------------
# a. forward and backward, no dropout, padded layout (and e: the exempt sentence of all_masked_p0)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_backward_against_float64(hip, arith, case):
    bf = arith == "bf16"
    x = AC.inputs(case, bf16=bf)
    got = launch(hip, arith, case, x)
    fig = Figures(f"a {case.name} {arith}")
    check_padded(fig, arith, case, got, ref_of(case.name, 0.0, bf, False))
    fig.settle()
    again = launch(hip, arith, case, x)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: second launch differs"


# ---------------------------------------------------------------------------------------------------------
# b. the zero-tail variants: dctx exactly zero behind each sentence's last unmasked position
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
def test_zero_tail_contract_against_float64(hip, arith, case):
    bf = arith == "bf16"
    x = AC.inputs(case, bf16=bf, zero_tail=True)
    got = launch(hip, arith, case, x, zero_tail=True)
    fig = Figures(f"b {case.name} {arith}")
    check_padded(fig, arith, case, got, ref_of(case.name, 0.0, bf, True))
    fig.settle()


# ---------------------------------------------------------------------------------------------------------
# c. dropout live
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_dropout_against_float64_under_the_replicated_mask(hip, arith, case, p):
    bf = arith == "bf16"
    x = AC.inputs(case, bf16=bf)
    got = launch(hip, arith, case, x, p=p)
    fig = Figures(f"c {case.name} {arith} p={p}")
    ref = ref_of(case.name, p, bf, False)
    check_padded(fig, arith, case, got, ref)
    fig.settle()
    # lse is that of the undropped scores: the reference's (compared above), and to the bit the kernel's own without dropout
    plain = launch(hip, arith, case, x)
    assert torch.equal(got["lse"], plain["lse"])


@pytest.mark.parametrize("name", ["s16_p0", "t106_two_holes"])
def test_kernel_draws_the_documented_mask(hip, arith, name):
    """The forward's keep pattern, read off a one-hot V slid over the key axis in windows of 64, is keep_mask: exactly, for
    every (sentence, head, query) and every unmasked key whose probability is not negligible; and a dropped key adds exactly
    nothing whatever its probability."""
    c, p = BY_NAME[name], 0.3
    B, S, P, NH, H, T = c.B, c.S, c.P, c.NH, c.H, c.T
    bf = arith == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    x = AC.inputs(c, bf16=bf)
    ref = ref_of(name, 0.0, bf, False)
    keep = torch.from_numpy(keep_of(name, p))
    live = (AC.mask_of(c) == 1)[:, None, None, :] & (ref["probs"] > 1e-6)
    assert float(live.double().mean()) > 0.2
    fwd = hip.prefix_attn_bf16_fwd if bf else hip.prefix_attn_fwd
    seen = torch.zeros(B, NH, S, T, dtype=torch.bool)
    kept = torch.zeros(B, NH, S, T, dtype=torch.bool)
    for w0 in range(0, T, 64):
        v = torch.zeros(B, NH, T, 64)
        for t in range(w0, min(w0 + 64, T)):
            v[:, :, t, t - w0] = 1.0
        qkv = x["qkv"].view(B, S, 3, NH, 64).clone()
        qkv[:, :, 2] = v[:, :, P:].permute(0, 2, 1, 3)
        ctx, lse = nans(B * S, H, dtype=dt), nans(B, NH, S)
        fwd(qkv.reshape(B * S, 3 * H).to(DEV).to(dt), x["pk"].to(DEV).to(dt) if P else None,
            v[:, :, :P].reshape(B, NH * P * 64).to(DEV).to(dt) if P else None, x["addmask"].to(DEV), ctx, lse, B, S, P, NH, p, SEED, OFFSET)
        torch.cuda.synchronize()
        pt = ctx.float().cpu().view(B, S, NH, 64).permute(0, 2, 1, 3)  # [B,NH,S,64] = Pd[..., w0 + d]
        n = min(64, T - w0)
        kept[..., w0:w0 + n] = pt[..., :n] > 0
        seen[..., w0:w0 + n] = True
    assert bool(seen.all())
    assert torch.equal(kept[live], keep[live]), f"{int((kept[live] != keep[live]).sum())} of {int(live.sum())} decisions differ"
    assert not bool(kept[~keep].any())
    # the comparison is not vacuous: both decisions occur among the n compared ones, at a rate that n draws of probability
    # 1 - p allow (5 standard deviations of the binomial; s16_p0 has 832 live decisions, sd 0.016)
    n = int(live.sum())
    frac = float(keep[live].double().mean())
    print(f"[attn-contract] mask {name} {arith}: {n} decisions equal, keep fraction {frac:.3f}")
    assert abs(frac - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5


# ---------------------------------------------------------------------------------------------------------
# d. packed rows, plain and ordered sentence list, without and with dropout
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["plain", "ordered"])
@pytest.mark.parametrize("case", [c for c in CASES if c.suffix_masked], ids=str)
def test_packed_layout_against_float64(hip, arith, case, order):
    c = case
    B, S, P, NH, H, T = c.B, c.S, c.P, c.NH, c.H, c.T
    bf = arith == "bf16"
    rows = AC.kept_rows(c)
    cu = AC.cu_plain(c) if order == "plain" else AC.cu_ordered(c)
    Mv, pad = len(rows), 37
    x = AC.inputs(c, bf16=bf, zero_tail=True)  # (a packed launch has no padded queries: their upstream gradient is zero)
    for p in (0.0, 0.3):
        got = launch(hip, arith, c, x, p=p, cu=cu, rows=rows, pad_rows=pad)
        ref = ref_of(c.name, p, bf, True)
        fig = Figures(f"d {c.name} {arith} {order} p={p}")
        for k in ("ctx", "dqkv", "dpk", "dpv"):
            if k in got:
                assert bool(torch.isfinite(got[k].float()).all()), k
        compare(fig, arith, c, "ctx", got["ctx"][:Mv], ref["ctx"][rows])
        compare(fig, arith, c, "dqkv", got["dqkv"][:Mv], ref["dqkv"][rows])
        if P:
            compare(fig, arith, c, "dpk", got["dpk"], ref["dpk"])
            compare(fig, arith, c, "dpv", got["dpv"], ref["dpv"])
        # the rows that pad the image: exact zeros
        assert float(got["ctx"][Mv:].float().abs().max()) == 0.0 and float(got["dqkv"][Mv:].float().abs().max()) == 0.0
        # lse / delta keep the [B, NH, S] indexing: compared on the kept queries
        qlive = torch.zeros(B, S, dtype=torch.bool)
        qlive.view(-1)[rows] = True
        qlive = qlive[:, None, :].expand(B, NH, S)
        compare(fig, arith, c, "lse", got["lse"].cpu()[qlive], ref["lse"][qlive])
        if not bf:
            compare(fig, arith, c, "delta", got["delta"].cpu()[qlive], ref["delta"][qlive])
        else:
            assert bool(torch.isfinite(got["partq"]).all()) and bool(torch.isfinite(got["partkv"]).all())
            sums = torch.cat([got["partq"].sum(0), got["partkv"].sum(0)]).double().cpu()
            nb, _ = BF16_GRAD.get(c.name, (1.2e-2, 2e-2))
            fig.add("partials(norm)", relerr(sums, ref["dqkv"][rows].sum(0)), nb)
            fig.add("partials-vs-stored", need(sums, got["dqkv"][:Mv].double().cpu().sum(0)), 2e-2)
        fig.settle()
