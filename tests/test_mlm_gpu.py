"""The masked-LM kernels on the MI355X (csrc/mlm.hip): mtvaf_mlm_mask bit for bit against the NumPy restatement, the chunked
vocabulary cross entropy (engine.VocabCEFunction) against float64, its invariance under the chunk width, its memory contract, and
BertForMaskedLM against the reference's golden vectors.

Bounds of the cross entropy, derived (nothing here is fitted to what the kernels give):
  logits   the GEMM bound tests/test_ops_gpu.py asserts, 2^-24 (4 + sqrt K) (|x| . |W|^T), plus one rounding of the bias add:
           E_ij = 2^-24 ((4 + sqrt H) mag_ij + |l_ij|), E_i = max_j E_ij
  row pass a shift of every logit by at most E_i moves the log-sum-exp by at most E_i and the label's logit by E_i; the row
           kernels add the margin of tests/test_token_ce_gpu.py for its log-sum-exp: |got - ref| <= 2 E_i + 1e-5 |ref| + 1e-6
  dlogits  D_ij = g_i p_ij (2 E_i + 1e-5) + 2^-23 |dl_ij|   (p = e^(l - lse): a relative error of the exponent's absolute one)
  dx       D . |W| + 2^-24 (4 + sqrt V + chunks) (|dl| . |W|)        (chunks: one rounding per accumulating product)
  dW       D^T . |x| + 2^-24 (4 + sqrt R) (|dl|^T . |x|);   dbias: colsum(D) + 2^-24 (4 + sqrt R) colsum(|dl|)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlm_cases as M
from test_model_gpu import DEV

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hip():
    from mtvaf_amd import hip as h
    h.lib()
    return h


# ---- masking -------------------------------------------------------------------------------------------------------------------
V_MASK, MASK_ID, SPECIAL = 97, 4, (0, 2, 3, 4)


def mask_case(name):
    rng = np.random.default_rng(len(name))
    B, S = 3, 70  # more than one wave per sentence
    ids = rng.integers(5, V_MASK, size=(B, S)).astype(np.int64)
    ids[:, 0] = 2
    lengths = [70, 41, 66]
    att = np.zeros((B, S), dtype=np.int64)
    for b, n in enumerate(lengths):
        att[b, :n] = 1
        ids[b, n - 1] = 3
        ids[b, n:] = 0
    u = rng.random((B, S, 3)).astype(np.float32)
    kw = dict(probability=0.3, special_mask=None, capacity=None)
    if name == "no_eligible_sentence":
        ids[1, :41] = 3
    elif name == "non_prefix_mask":
        att[0, 5:9] = 0
        att[2, ::3] = 0
        att[1, 50:60] = 1  # live tokens behind a gap (their ids are the pad id: special)
        ids[1, 52:55] = 9
    elif name == "special_mask":
        sm = (rng.random((B, S)) < 0.4).astype(np.int64)
        kw["special_mask"] = sm
    elif name == "u0_at_probability":
        kw["probability"] = 0.25
        u[0, 3:20, 0] = np.float32(0.25)            # not selected: the comparison is strict
        u[0, 20:30, 0] = np.nextafter(np.float32(0.25), np.float32(0))
    elif name == "random_id_top":
        u[..., 0] = 0.0
        u[..., 1] = 0.85
        u[0, :, 2] = np.nextafter(np.float32(1), np.float32(0))  # int(u2 V) = V in fp32: clipped to V - 1
        u[1, :, 2] = 0.0
    elif name == "capacity_short":
        kw["capacity"] = 16
    elif name == "capacity32_none_selected":
        kw["capacity"], kw["probability"] = 32, 0.0
    return ids, att, u, kw


@pytest.mark.parametrize("name", ["plain", "no_eligible_sentence", "non_prefix_mask", "special_mask", "u0_at_probability",
                                  "random_id_top", "capacity_short", "capacity32_none_selected"])
def test_mask_tokens_equals_the_restatement(hip, name):
    from mtvaf_amd import mlm
    ids, att, u, kw = mask_case(name)
    cap = kw["capacity"] if kw["capacity"] is not None else mlm.default_capacity(ids.size, kw["probability"])
    want = M.mask_reference(ids, att, u, kw["probability"], MASK_ID, V_MASK, SPECIAL, kw["special_mask"], cap)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    run = lambda: mlm.mask_tokens(dev(ids), dev(att), mask_token_id=MASK_ID, vocab_size=V_MASK, special_ids=SPECIAL,
                                  probability=kw["probability"], capacity=kw["capacity"], special_mask=dev(kw["special_mask"]),
                                  uniforms=dev(u))
    got, again = run(), run()
    assert torch.equal(got["input_ids"].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(got["positions"].cpu(), torch.from_numpy(want[1]))
    assert torch.equal(got["labels"].cpu(), torch.from_numpy(want[2]))
    assert got["count"].tolist() == [want[3]] and got["stats"].tolist() == want[4].tolist()
    for k in ("input_ids", "positions", "labels", "count", "stats"):
        assert torch.equal(got[k], again[k])
    if name == "capacity_short":
        assert want[4][2] > 0
    if name == "capacity32_none_selected":
        assert want[3] == 0 and cap == 32
    if name == "random_id_top":
        assert (want[0][0, 1:69] == V_MASK - 1).all() and (want[0][1, 1:40] == 0).all()
    if name == "u0_at_probability":
        assert not np.isin(np.arange(3, 20), want[1]).any() and np.isin(np.arange(20, 30), want[1]).all()


def test_mask_tokens_draws_its_own_uniforms(hip):
    from mtvaf_amd import engine, mlm
    ids, att, _, _ = mask_case("plain")
    torch.manual_seed(11)
    off = engine.RNG.offset
    out = mlm.mask_tokens(torch.from_numpy(ids).to(DEV), torch.from_numpy(att).to(DEV), mask_token_id=MASK_ID, vocab_size=V_MASK,
                          special_ids=SPECIAL, probability=0.5)
    assert engine.RNG.offset == off + 1  # one offset per call
    u = out["uniforms"].cpu().numpy()
    assert u.shape == (3, 70, 3) and (u >= 0).all() and (u < 1).all() and 0.4 < u.mean() < 0.6 and len(np.unique(u)) > 600
    want = M.mask_reference(ids, att, u, 0.5, MASK_ID, V_MASK, SPECIAL, None, out["positions"].numel())
    assert torch.equal(out["input_ids"].cpu(), torch.from_numpy(want[0])) and out["count"].tolist() == [want[3]]


def test_gather_rows_and_its_backward(hip):
    from mtvaf_amd import mlm
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(3, 7, 64, generator=g).to(DEV).requires_grad_(True)
    pos = torch.tensor([0, 5, 6, 20, -1, -1], dtype=torch.int32, device=DEV)
    rows = mlm.gather_rows(hidden, pos)
    flat = hidden.detach().view(-1, 64)
    assert torch.equal(rows[:4], flat[pos[:4].long()]) and not bool(rows[4:].any())
    up = torch.randn(6, 64, generator=g).to(DEV)
    rows.backward(up)
    want = torch.zeros(21, 64, device=DEV)
    want[pos[:4].long()] = up[:4]
    assert torch.equal(hidden.grad.view(-1, 64), want)


# ---- vocabulary cross entropy ----------------------------------------------------------------------------------------------------
CAP, COUNT, H, V = 40, 29, 64, 1037
CHUNKS = (256, V, 32)  # five chunks, the last 13 wide; one chunk; 33 chunks


@pytest.fixture(scope="module")
def ce_case():
    """Inputs and the float64 reference, computed once."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(CAP, H, generator=g)
    W = torch.randn(V, H, generator=g) * 0.3
    bias = torch.randn(V, generator=g) * 0.5
    labels = torch.randint(0, V, (CAP,), generator=g)
    labels[0], labels[1], labels[2] = 0, V - 1, 1030            # the ends; inside the last partial chunk of 256
    x[3] = 6.0 * W[700] / W[700].norm()                          # maximum in the chunk of column 700 ...
    labels[3] = 5                                                # ... the label in another
    labels[4], labels[5] = V + 3, -100                           # out of range; ignored
    W[600], bias[600] = W[100], bias[100]                        # two identical columns in different chunks (at 256 and at 32)
    x[7] = 8.0 * W[100] / W[100].norm()                          # ... which are row 7's maximum: an exact tie
    labels[7] = 600                                              # the LATER one: the first argmax is 100, not correct
    x[8] = 8.0 * W[300] / W[300].norm()
    labels[8] = 300                                              # a row that is correct
    z = x.double() @ W.double().t()
    x[6] *= 1e4 / float(z[6].abs().max())                        # logits at +-1e4
    z = x.double() @ W.double().t() + bias.double()
    ref = M.ce_oneshot(z.numpy(), labels.numpy(), COUNT)
    assert ref["argmax"][7] == 100 and ref["argmax"][3] == 700 and 9e3 < np.abs(z[6].numpy()).max() < 1.1e4
    mag = x.double().abs() @ W.double().abs().t()
    E = (2.0 ** -24 * ((4 + H ** 0.5) * mag + z.abs())).max(1).values.numpy()
    return {"x": x, "W": W, "bias": bias, "labels": labels, "z": z, "ref": ref, "E": E}


def run_ce(case, chunk, reduction="mean", upstream=None, count=COUNT):
    from mtvaf_amd import engine
    x, W, b = (case[k].to(DEV).requires_grad_(True) for k in ("x", "W", "bias"))
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    loss, rows, lse, stats = engine.VocabCEFunction.apply(x, W, b, case["labels"].to(DEV), cnt, reduction, chunk)
    if reduction == "none":
        rows.backward(upstream.to(DEV))
    else:
        loss.backward(None if upstream is None else torch.tensor(upstream, device=DEV))
    return {"loss": loss.detach(), "rows": rows.detach(), "lse": lse, "stats": stats, "dx": x.grad, "dW": W.grad, "db": b.grad}


def grad_bounds(case, g_rows, chunk):
    x, W, z = case["x"].double(), case["W"].double(), case["z"]
    labels, E = case["labels"].numpy(), case["E"]
    dl = torch.from_numpy(M.ce_grad_logits(z.numpy(), labels, COUNT, g_rows))
    live = torch.from_numpy(M._live(labels, COUNT, V))
    p = torch.softmax(z, 1) * live[:, None]
    D = torch.from_numpy(np.abs(g_rows))[:, None] * p * torch.from_numpy(2 * E + 1e-5)[:, None] + 2.0 ** -23 * dl.abs()
    nchunks = -(-V // chunk)
    ref = {"dx": dl @ W, "dW": dl.t() @ x, "db": dl.sum(0)}
    tol = {"dx": D @ W.abs() + 2.0 ** -24 * (4 + V ** 0.5 + nchunks) * (dl.abs() @ W.abs()),
           "dW": D.t() @ x.abs() + 2.0 ** -24 * (4 + CAP ** 0.5) * (dl.abs().t() @ x.abs()),
           "db": D.sum(0) + 2.0 ** -24 * (4 + CAP ** 0.5) * dl.abs().sum(0)}
    return ref, tol, live


def check_grads(case, got, g_rows, chunk):
    ref, tol, live = grad_bounds(case, g_rows, chunk)
    for k in ("dx", "dW", "db"):
        g = got[k].double().cpu()
        assert bool(torch.isfinite(g).all()), k
        err = (g - ref[k]).abs()
        worst = float((err / tol[k].clamp(min=1e-300)).max())
        print(f"chunk {chunk} {k}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
        assert bool((err <= tol[k]).all()), (k, worst)
    assert not bool(got["dx"].cpu()[~live].any())  # rows >= count, the ignored and the out-of-range row: exact zeros


@pytest.mark.parametrize("chunk", CHUNKS)
def test_vocab_ce_against_float64(hip, ce_case, chunk):
    ref, E = ce_case["ref"], ce_case["E"]
    got = run_ce(ce_case, chunk)
    rows, lse = got["rows"].double().cpu().numpy(), got["lse"].double().cpu().numpy()
    assert np.isfinite(rows).all() and np.isfinite(lse).all()
    live = M._live(ce_case["labels"].numpy(), COUNT, V)
    for name, g, r in (("loss_row", rows, ref["loss_row"]), ("lse_row", lse, ref["lse_row"])):
        err, allowed = np.abs(g - r), 2 * E * live + 1e-5 * np.abs(r) + 1e-6
        print(f"chunk {chunk} {name}: max err {err.max():.3e}, worst err / bound {(err / allowed).max():.3f}")
        assert (err <= allowed).all(), name
    assert not rows[~live].any() and not lse[~live].any()
    loss_tol = float((2 * E * live).sum() / ref["live"] + 1e-5 * abs(ref["loss"]) + 1e-6)
    print(f"chunk {chunk} loss: err {abs(float(got['loss']) - ref['loss']):.3e}, bound {loss_tol:.3e}")
    assert abs(float(got["loss"]) - ref["loss"]) <= loss_tol
    assert got["stats"].tolist() == [ref["live"], ref["correct"], 1]  # 27 live rows; the tie row is not correct; one bad label
    check_grads(ce_case, got, np.full(CAP, 1.0 / ref["live"]), chunk)


def test_vocab_ce_sum_and_per_row_upstream(hip, ce_case):
    ref = ce_case["ref"]
    got = run_ce(ce_case, 256, "sum", upstream=0.5)
    live = M._live(ce_case["labels"].numpy(), COUNT, V)
    tol = float((2 * ce_case["E"] * live).sum() + 1e-5 * abs(ref["loss_row"].sum()) + 1e-6)
    assert abs(float(got["loss"]) - ref["loss_row"].sum()) <= tol
    check_grads(ce_case, got, np.full(CAP, 0.5), 256)
    up = torch.linspace(-1.0, 2.0, CAP)
    got = run_ce(ce_case, 256, "none", upstream=up)
    check_grads(ce_case, got, up.double().numpy(), 256)


def test_vocab_ce_without_live_rows(hip, ce_case):
    got = run_ce(ce_case, 256, count=0)
    assert float(got["loss"]) == 0.0 and not np.signbit(float(got["loss"])) and got["stats"].tolist() == [0, 0, 0]
    for k in ("dx", "dW", "db", "rows", "lse"):
        assert not bool(got[k].any()) and bool(torch.isfinite(got[k]).all()), k


def run_state(hip, case, chunk):
    """The chunk loop on the ABI, on NaN-prefilled buffers -> (loss, loss_row, lse_row, stats, first argmax)"""
    x, W, b, lab = (case[k].to(DEV) for k in ("x", "W", "bias", "labels"))
    cnt = torch.tensor([COUNT], dtype=torch.int32, device=DEV)
    state = torch.full((4 * CAP,), float("nan"), device=DEV)
    for v0 in range(0, V, chunk):
        v1 = min(V, v0 + chunk)
        lg = torch.full((CAP, v1 - v0), float("nan"), device=DEV)
        hip.linear_fwd(x, W[v0:v1], None, lg)
        hip.vocab_ce_chunk_fwd(lg, b, lab, cnt, state, V, v0, v1)
    loss, rows, lse = (torch.full((n,), float("nan"), device=DEV) for n in (1, CAP, CAP))
    stats = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    hip.vocab_ce_finish(state, lab, cnt, loss, rows, lse, stats, V, hip.VOCAB_CE_REDUCTIONS["mean"])
    return loss, rows, lse, stats, state[3 * CAP:].view(torch.int32).clone()


def test_chunk_invariance_and_determinism(hip, ce_case):
    live = torch.from_numpy(M._live(ce_case["labels"].numpy(), COUNT, V))
    runs = {c: run_state(hip, ce_case, c) for c in CHUNKS}
    base = runs[V]
    margin = lambda r: 1e-5 * r.abs() + 1e-6  # the row pass alone: the logits are the same products at every width
    for c in (32, 256):
        loss, rows, lse, stats, arg = runs[c]
        assert torch.equal(arg[live], base[4][live]) and torch.equal(stats, base[3])  # the argmax is identical
        for name, a, b in (("lse_row", lse, base[2]), ("loss_row", rows, base[1]), ("loss", loss, base[0])):
            err = (a - b).abs().cpu()
            print(f"chunk {c} vs {V} {name}: max err {float(err.max()):.3e}")
            assert bool((err <= margin(b.cpu())).all()), (c, name)
    assert int(base[4][7]) == 100 and int(base[4][3]) == 700
    for c in CHUNKS:  # repeated runs: the same bits in every output
        again = run_state(hip, ce_case, c)
        for a, b in zip(runs[c], again):  # (the argmax words of dead rows keep their prefill: the same bits too)
            assert torch.equal(a, b)
    a, b = run_ce(ce_case, 256), run_ce(ce_case, 256)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_memory_contract(hip):
    from mtvaf_amd import engine, mlm
    R = mlm.default_capacity(32 * 128, 0.15)
    c = engine.VOCAB_CE_CHUNK
    assert hip.vocab_ce_workspace_bytes(R, 768, 30522, c) == hip.vocab_ce_workspace_bytes(R, 768, 2 * 30522, c)
    assert hip.vocab_ce_workspace_bytes(R, 768, 30522, c) < 4 * R * 30522
    assert hip.vocab_ce_workspace_bytes(R, 768, 30522, c) <= 4 * R * c + 16 * R + 512


# ---- head and model --------------------------------------------------------------------------------------------------------------
def test_bert_for_masked_lm_matches_the_reference_golden(hip):
    import mlm_model_check
    mlm_model_check.check()


def test_bert_for_masked_lm_with_gradients_returned_through_autograd():
    """MTVAF_DIRECT_GRADS is read when the engine is imported: the same check in a child process with the switch at 0."""
    env = dict(os.environ, MTVAF_DIRECT_GRADS="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "mlm_model_check.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "direct_grads=False" in r.stdout and r.stdout.strip().endswith("ok")
