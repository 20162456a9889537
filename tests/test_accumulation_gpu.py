"""Fused gradient accumulation on the MI355X.

The criterion everywhere is ONE fp32 add: an accumulating launch forms the value its overwriting form stores -- same MFMA order, same
summation order -- and adds the destination's old value once, last.  IEEE addition is commutative, so ``old + new`` has one bit
pattern and every comparison below is ``torch.equal``; no tolerance is chosen anywhere except where an optimizer trajectory is compared
with the fallback's (the tolerances of test_optim_gpu.test_build_optimizer_with_gradient_accumulation_equals_torch_adamw, with its
two exclusions)."""
import types

import pytest
import torch

from test_js_consistency_gpu import _batch as cut_batch, _build as cut_build, fixed_cut  # noqa: F401  (fixture)
from test_ops_gpu import DEV, hip, rnd  # noqa: F401  (fixture)
from test_optim_gpu import _batch, _model

pytestmark = pytest.mark.gpu


# ---- 1. kernels ------------------------------------------------------------------------------------------------------
def _padded(M, N, seed):
    """A destination [M, N] inside a larger random buffer (two extra rows, leading dimension N + 8): -> (whole, view)."""
    whole = rnd(M + 2, N + 8, seed=seed).to(DEV)
    return whole, whole[1:M + 1, 4:N + 4]


def _check_group(run, shapes, seed):
    """run(outs, accumulate): the grouped launch into `outs`.  Overwriting form into a, accumulating form onto a random prior c0:
    out == c0 + a bit for bit, and nothing outside the products' rows and columns moves."""
    a_w = [_padded(M, N, seed + i) for i, (M, N) in enumerate(shapes)]
    run([v for _, v in a_w], False)
    c_w = [_padded(M, N, seed + 50 + i) for i, (M, N) in enumerate(shapes)]
    before = [w.clone() for w, _ in c_w]
    run([v for _, v in c_w], True)
    torch.cuda.synchronize()
    for i, ((M, N), (_, a), (w, c), b) in enumerate(zip(shapes, a_w, c_w, before)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(c, b[1:M + 1, 4:N + 4] + a), f"product {i} {M}x{N}: not one add away from the overwriting form"
        keep = torch.ones_like(w, dtype=torch.bool)
        keep[1:M + 1, 4:N + 4] = False
        assert torch.equal(w[keep], b[keep]), f"product {i}: the padding of the destination moved"


# every tile form of the grouped pre-split launch once: N multiples of 128 only (384 = 2 x 192 among them: the 192-column tile serves
# forward products only, a grouped launch never takes it) -> the 128 x 128 kernel; all N multiples of 256 -> the 128 x 256 kernel
PLANES_SHAPES = {"n128": [(128, 384), (256, 128), (128, 128), (384, 128)], "n256": [(128, 256), (256, 512), (384, 256), (128, 256)]}


@pytest.mark.parametrize("K", [32, 96])  # (the ring's prologue alone / prologue + steady state + drain)
@pytest.mark.parametrize("form", ["n128", "n256"])
@pytest.mark.parametrize("jobs", [False, True])
def test_planes_group_accumulates_with_one_add(hip, form, K, jobs):
    shapes = PLANES_SHAPES[form]
    dys = [rnd(K, M, seed=10 + i).to(DEV) for i, (M, _) in enumerate(shapes)]
    xs = [rnd(K, N, seed=20 + i).to(DEV) for i, (_, N) in enumerate(shapes)]
    pas, pbs = [hip.Planes(t, True) for t in dys], [hip.Planes(t, True) for t in xs]
    Hh = 200
    part = rnd(37, 3 * Hh, seed=30).to(DEV)  # the LayerNorm layout: partial rows [G][3][H], a job per column block, ld = 3H
    src2 = rnd(K, 384, seed=31).to(DEV)
    cs_a = [torch.full((Hh,), float("nan"), device=DEV) for _ in range(3)] + [torch.full((384,), float("nan"), device=DEV)]
    cs_c = [rnd(Hh, seed=40 + i).to(DEV) for i in range(3)] + [rnd(384, seed=43).to(DEV)]
    cs_before = [t.clone() for t in cs_c]

    def run(outs, accumulate):
        cs = cs_c if accumulate else cs_a
        colsum = [(part[:, j * Hh:(j + 1) * Hh], cs[j]) for j in range(3)] + [(src2, cs[3])] if jobs else None
        hip.gemm_planes_dw_group(list(zip(pas, pbs, outs)), colsum=colsum, accumulate=accumulate)

    _check_group(run, shapes, seed=100)
    if jobs:
        for a, c, b in zip(cs_a, cs_c, cs_before):
            assert torch.equal(c, b + a)
    # which kernel ran is the launch's own rule: the wide mask admits the 256-column tile for weight gradients by default
    assert hip.f32p_wide() & 4


def test_planes_group_without_the_flag_is_the_old_entry(hip):
    K, shapes = 64, PLANES_SHAPES["n256"]
    pas = [hip.Planes(rnd(K, M, seed=10 + i).to(DEV), True) for i, (M, _) in enumerate(shapes)]
    pbs = [hip.Planes(rnd(K, N, seed=20 + i).to(DEV), True) for i, (_, N) in enumerate(shapes)]
    a = [torch.full((M, N), float("nan"), device=DEV) for M, N in shapes]
    b = [torch.full((M, N), float("nan"), device=DEV) for M, N in shapes]
    hip.gemm_planes_dw_group(list(zip(pas, pbs, a)))
    hip.gemm_planes_dw_group(list(zip(pas, pbs, b)), accumulate=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


SK_FOUR = [(256, 512), (512, 256), (256, 256), (768, 256)]  # 14 tiles of unequal products


@pytest.mark.parametrize("shapes,T,shared", [([(256, 256)], 1024, True), (SK_FOUR, 1024, True), (SK_FOUR, 512, False)],
                         ids=["one-tile-1024-rows-shared", "four-products-1024-rows-shared", "four-products-512-rows-whole-tiles"])
def test_bf16_stream_k_group_accumulates_with_one_add(hip, shapes, T, shared):
    """The cut is the planner's (p256_plan: S pieces per tile, S | KT, KT / S >= 3, all pieces in one round of the CUs) and is ASKED
    for, not assumed (mtvaf_gemm_bf16x_dw_group_pieces, the launch's own planner call).  512 token rows are 8 k-tiles: only S = 1 or 2
    are admitted and S = 1 is cheaper (8 x 1.55 + 6.5 = 18.9 us against 4 x 1.55 + 13.5 = 19.7), so every block owns a whole tile and
    adds the old value in the plain epilogue.  1024 rows are 16 k-tiles: S = 4 (19.7 us against 31.3 unsplit) -- three blocks of a
    tile store contributions and never read the destination, the fourth combines them in k order and THEN adds the old value."""
    assert hip.streamk_ensure(DEV)
    pieces = hip.gemm_bf16x_dw_group_pieces(shapes, T, DEV)
    assert pieces >= 1 and (pieces > 1) == shared, f"planner cut: {pieces} piece(s) per tile"
    dys = [rnd(T, M, seed=10 + i).to(torch.bfloat16).to(DEV) for i, (M, _) in enumerate(shapes)]
    xs = [rnd(T, N, seed=20 + i).to(torch.bfloat16).to(DEV) for i, (_, N) in enumerate(shapes)]
    _check_group(lambda outs, acc: hip.gemm_bf16x_dw_group(list(zip(dys, xs, outs)), T, accumulate=acc), shapes, seed=200)
    assert hip.streamk_error(DEV) == 0


@pytest.mark.parametrize("K,split", [(256, False), (256, True), (2048, True)])
@pytest.mark.parametrize("splits", [-1, 2])
def test_f32_group_accumulates_with_one_add(hip, K, split, splits):
    """mtvaf_gemm_f32_dw_group_acc: the pipe's 128 x 96 ring (K <= 1024 or the pipe arithmetic) and the split kernel's group form
    (split arithmetic, K > 1024: bias sums taken inside the launch when unsplit), planned and forced split counts, with bias sums."""
    shapes = [(128, 384), (256, 384), (128, 384), (384, 384)]
    dys = [rnd(K, M, seed=10 + i).to(DEV) for i, (M, _) in enumerate(shapes)]
    xs = [rnd(K, N, seed=20 + i).to(DEV) for i, (_, N) in enumerate(shapes)]
    db_a = [None, torch.full((256,), float("nan"), device=DEV), None, torch.full((384,), float("nan"), device=DEV)]
    db_c = [None, rnd(256, seed=41).to(DEV), None, rnd(384, seed=43).to(DEV)]
    db_before = [None if t is None else t.clone() for t in db_c]
    was = hip.f32_split()
    try:
        hip.f32_split(split)
        _check_group(lambda outs, acc: hip.gemm_f32_dw_group(list(zip(dys, xs, outs)), K, splits=splits, dbias=db_c if acc else db_a,
                                                             accumulate=acc), shapes, seed=300)
    finally:
        hip.f32_split(was)
    for a, c, b in zip(db_a, db_c, db_before):
        if a is not None:
            assert torch.equal(c, b + a)


# ---- 2. executor: every branch of mtvaf_encoder_layer_bwd --------------------------------------------------------------
def _encoder(H, NH, I, L=1):
    from transformers import BertConfig
    from mtvaf_amd.models.modeling_bert import BertEncoder
    cfg = BertConfig(vocab_size=64, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                     max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(7)
    enc = BertEncoder(cfg).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "LayerNorm.weight" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    return enc.eval()


# branch -> (compute, H, NH, I, B, S, packed rows?, module switches)
BRANCHES = {
    "fp32-ungrouped": ("fp32", 128, 2, 256, 4, 32, False, {}),
    "fp32-grouped": ("fp32", 384, 6, 768, 4, 32, False, {}),
    "fp32-planes": ("fp32", 128, 2, 256, 16, 64, True, {}),
    "bf16-ungrouped": ("bf16", 128, 2, 256, 4, 64, False, {}),
    "bf16-grouped": ("bf16", 256, 4, 512, 16, 64, False, {}),  # 1024 token rows: the stream-K group shares its tiles between blocks
}
GROUP_KEYS = {"fp32-grouped": {1012, 1225}, "fp32-planes": {428, 460}, "bf16-grouped": {777}}


@pytest.mark.parametrize("branch", list(BRANCHES))
def test_executor_accumulates_all_sixteen_gradients(hip, branch, monkeypatch):
    """One layer, one graph, backward twice: overwriting, then accumulating on top.  All sixteen parameter gradients == g + g bit
    for bit; the gradients of the activations (hidden input, prefix keys / values) are those of the single call -- autograd adds the
    second one itself, so they read 2 x the first exactly."""
    from mtvaf_amd import engine
    from mtvaf_amd.models.modeling_bert import PrefixKV
    compute, H, NH, I, B, S, packed, switches = BRANCHES[branch]
    for k, v in switches.items():
        monkeypatch.setattr(engine, k, v)
    was = hip.COMPUTE
    hip.set_compute_dtype(compute)
    try:
        enc = _encoder(H, NH, I)
        Pn = 4
        lengths = [S] * B if not packed else [S - (3 * i) % 9 for i in range(B)]
        mask = torch.zeros(B, Pn + S, device=DEV)
        for b, n in enumerate(lengths):
            mask[b, Pn + n:] = -10000.0
        valid = (mask[:, Pn:] == 0).float()[..., None]
        h0 = rnd(B, S, H, seed=1).to(DEV).requires_grad_(True)
        flat = (0.5 * rnd(1, 2, B, Pn * H, seed=2)).to(DEV).requires_grad_(True)
        w = rnd(B, S, H, seed=3).to(DEV) * valid  # (masked positions carry exactly-zero gradients: the contract of unpad_ok)
        sink = enc.grad_sink
        out = enc(h0, attention_mask=mask, past_key_values=PrefixKV(flat, NH, 64), unpad_ok=packed).last_hidden_state
        loss = (out * w).sum()
        hip.prof_start(256)
        loss.backward(retain_graph=True)
        cfgs = {r[0]["cfg"] for r in hip.prof_stop(256)}
        torch.cuda.synchronize()
        if branch == "bf16-grouped":
            assert hip.gemm_bf16x_dw_group_pieces([(H, I), (I, H), (H, H), (3 * H, H)], B * S, DEV) > 1, "tiles shared between blocks"
        if branch in GROUP_KEYS:
            assert cfgs & GROUP_KEYS[branch], (branch, sorted(cfgs))
        else:
            assert not cfgs & {1012, 1225, 428, 460, 777}, (branch, sorted(cfgs))
        assert sink.fast and not sink.accumulate
        params = [p for p in enc.layer[0].ordered_params()]
        g = [p.grad.clone() for p in params]
        dh, dpkv = h0.grad.clone(), flat.grad.clone()
        assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in g + [dh, dpkv])
        sink.accumulate_passes = 2
        sink._pass = 1
        loss.backward()
        torch.cuda.synchronize()
        assert sink.fast and sink.accumulate, "the second pass found its own flat views and added into them"
        for i, (p, gi) in enumerate(zip(params, g)):
            assert torch.equal(p.grad, gi + gi), f"{branch}: parameter gradient {i} is not g + g"
        assert torch.equal(h0.grad, dh + dh) and torch.equal(flat.grad, dpkv + dpkv)
    finally:
        hip.set_compute_dtype(was)


# ---- 3. model: k = 2 micro-batches, fused against the fallback in the same process ---------------------------------------
def _enc_grads(m):
    return {n: p.grad.clone() for n, p in m.bert.encoder.named_parameters()}


MODES = ["fp32", "fp32-planes", "bf16-group"]
MODE_KEYS = {"fp32": set(), "fp32-planes": {428, 460}, "bf16-group": {777}}  # the grouped weight-gradient launch a mode must take
ALL_GROUP_KEYS = {1012, 1225, 428, 460, 777}


def _build_mode(hip, mode, monkeypatch):
    """-> (model in eval mode, cfg, B, S).  fp32: 128 token rows, ungrouped; fp32-planes: 16 x 64 packed rows >= 512, plane images;
    bf16-group: H = 256 / I = 512 at 1024 PADDED token rows (a packed row count need not be whole 256-row tiles), the stream-K group
    with tiles shared between blocks.  The caller restores hip.COMPUTE."""
    import params as P
    from test_model_gpu import LABELS, hf_config, make_args
    if mode == "bf16-group":
        from mtvaf_amd import engine
        hip.set_compute_dtype("bf16")
        monkeypatch.setattr(engine, "UNPAD", False)
        from mtvaf_amd.models.bert_model import TVNetSAModel2
        cfg = P.EncCfg(vocab_size=600, hidden=256, heads=4, inter=512, layers=2, max_pos=64)
        args = make_args(alpha=0.0)
        args.bert_config = hf_config(cfg, dropout=0.0)
        torch.manual_seed(11)
        m = TVNetSAModel2(LABELS, None, args).to(DEV)
        B, S = 16, 64
        assert hip.gemm_bf16x_dw_group_pieces([(256, 512), (512, 256), (256, 256), (768, 256)], B * S, DEV) > 1
    else:
        hip.set_compute_dtype("fp32")
        m, cfg = _model(layers=2)
        B, S = (16, 64) if mode == "fp32-planes" else (4, 32)
    return m.eval(), cfg, B, S


def _profiled(hip, fn):
    """fn() under the launch profiler -> (its result, the set of GEMM launch keys it made)."""
    hip.prof_start(4096)
    try:
        out = fn()
    finally:
        cfgs = {r[0]["cfg"] for r in hip.prof_stop(4096)}
    return out, cfgs


def _check_branch(mode, cfgs):
    if MODE_KEYS[mode]:
        assert cfgs & MODE_KEYS[mode], f"{mode}: its grouped weight-gradient launch did not run ({sorted(cfgs)})"
    assert not (cfgs & ALL_GROUP_KEYS) - MODE_KEYS[mode], f"{mode}: another branch's grouped launch ran ({sorted(cfgs)})"


def _two_micro_batches(m, cfg, B, S, fused):
    sink = m.bert.encoder.grad_sink
    sink.accumulate_passes = 2 if fused else 0
    sink.reset_passes()
    m.zero_grad(set_to_none=True)
    fast = []
    for seed in (5, 9):
        (m(**_batch(cfg, B=B, S=S, seed=seed)).loss / 2).backward()
        fast.append((sink.fast, sink.accumulate))
    torch.cuda.synchronize()
    sink.accumulate_passes = 0
    return _enc_grads(m), fast


@pytest.mark.parametrize("mode", MODES)
def test_model_two_micro_batches_equal_the_fallback_bit_for_bit(hip, mode, monkeypatch):
    was = hip.COMPUTE
    try:
        m, cfg, B, S = _build_mode(hip, mode, monkeypatch)
        ref, fast0 = _two_micro_batches(m, cfg, B, S, fused=False)
        (got, fast1), cfgs = _profiled(hip, lambda: _two_micro_batches(m, cfg, B, S, fused=True))
        _check_branch(mode, cfgs)
        if mode == "fp32-planes":
            assert m.bert.encoder._stores[0].weights._pl is not None, "the weights' plane images exist: the plane-image path ran"
        assert fast0 == [(True, False), (False, False)], "the fallback is what it was"
        assert fast1 == [(True, False), (True, True)], "the second micro-batch added into the flat buffers"
        assert all(p.grad is not None for p in m.bert.encoder.parameters())
        for n, r in ref.items():
            assert torch.equal(got[n], r), f"{mode}: {n}"
    finally:
        hip.set_compute_dtype(was)


@pytest.mark.parametrize("mode", MODES)
def test_overlap_with_accumulation_steps_equals_the_fallback_schedule(hip, mode, monkeypatch):
    """On the ungrouped fp32 shape, with plane images (rewritten behind the in-backward update of the last accumulating pass) and
    in the mixed-precision mode (its bf16 shadow rewritten there).  Two optimizer steps of two micro-batches each:
    AdamW(overlap=True, accumulation_steps=2) -- pass 1 adds and updates nothing,
    pass 2 updates each layer from inside its backward -- against build_optimizer's fallback (overlap=False).  Tolerances and the two
    exclusions of test_optim_gpu.test_build_optimizer_with_gradient_accumulation_equals_torch_adamw.  A third backward raises."""
    import copy
    from mtvaf_amd.optim import AdamW, build_optimizer, reference_param_groups
    was = hip.COMPUTE
    try:
        m, cfg, B, S = _build_mode(hip, mode, monkeypatch)
        _accumulation_trajectory(hip, mode, m, cfg, B, S, copy.deepcopy(m))
    finally:
        hip.set_compute_dtype(was)
    if mode != "fp32":
        return
    batches = [_batch(cfg, seed=5), _batch(cfg, seed=9)]
    # overlap=False with k > 1 simply shares the flat buffers; step() then updates the layers from them
    m2, _ = _model(layers=2)
    m2.eval()
    o2 = AdamW(reference_param_groups(m2, 1e-3), model=m2, overlap=False, accumulation_steps=2)
    s2 = m2.bert.encoder.grad_sink
    for b in batches:
        (m2(**b).loss / 2).backward()
    assert s2.fast and s2.accumulate and s2.on_layer_done is None
    o2.step()


def _accumulation_trajectory(hip, mode, m, cfg, B, S, ref):
    from mtvaf_amd.optim import build_optimizer
    args = types.SimpleNamespace(lr=1e-3, warmup_ratio=0.0, use_prefix=True, gradient_accumulation_steps=2)
    ropt, _ = build_optimizer(ref, args, 100)
    assert ropt.overlap is False and ref.bert.encoder.grad_sink.accumulate_passes == 0
    args.fused_accumulation = True
    opt, _ = build_optimizer(m, args, 100)
    sink = m.bert.encoder.grad_sink
    assert opt.overlap is True and opt.accumulation_steps == 2 and sink.accumulate_passes == 2 and sink.on_layer_done is not None
    batches = [_batch(cfg, B=B, S=S, seed=5), _batch(cfg, B=B, S=S, seed=9)]
    w0 = m.bert.encoder.layer[0].intermediate.dense.weight
    for mod, o in ((m, opt), (ref, ropt)):
        for step in range(2):
            for i, b in enumerate(batches):
                before = w0.detach().clone()
                if mod is m and step == 1 and i == 1:  # (the last accumulating pass of a step whose forward read updated weights)
                    _, cfgs = _profiled(hip, lambda: (mod(**b).loss / 2).backward())
                    _check_branch(mode, cfgs)
                else:
                    (mod(**b).loss / 2).backward()
                if mod is m:
                    torch.cuda.synchronize()
                    assert sink.fast and sink.accumulate == (i == 1)
                    assert torch.equal(w0, before) == (i == 0), "updated from inside the LAST backward, and only there"
            o.step()
            o.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if "key.bias" in n or "word_embeddings" in n:
            continue  # pure-noise gradient whose sign Adam amplifies / float-atomic scatter-add
        atol = 2.5e-4 if (n.startswith("crf") or n.startswith("fc")) else 5e-6
        torch.testing.assert_close(p, q, rtol=0, atol=atol, msg=n)
    for b in batches:
        (m(**b).loss / 2).backward()
    with pytest.raises(RuntimeError, match="second backward"):
        (m(**batches[0]).loss / 2).backward()
    opt.step()


# ---- 4. the cutoff step: two encoder nodes under one backward --------------------------------------------------------------
def test_cutoff_step_shares_the_flat_buffers(fixed_cut):
    from mtvaf_amd.optim import AdamW
    m, args = cut_build(True)
    m.eval()
    batch = cut_batch(True)
    sink = m.bert.encoder.grad_sink
    m.forward_with_cutoff(**batch).loss.backward()  # the tree's behaviour without the opt-in: both nodes fall back
    torch.cuda.synchronize()
    assert sink.fast is False
    ref = _enc_grads(m)
    m.zero_grad(set_to_none=True)
    args.fused_accumulation = True
    out = m.forward_with_cutoff(**batch)
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (1, 2)
    out.loss.backward()
    torch.cuda.synchronize()
    assert sink.fast is True and sink.accumulate is True
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (0, 1), "back to its setting when the pass ended"
    got = _enc_grads(m)
    for n, r in ref.items():  # (the sum of two values has one bit pattern, whichever node ran first)
        assert torch.equal(got[n], r), n
    views = [v for st in m.bert.encoder._stores for v in st.grad_views()]
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip([p for l in m.bert.encoder.layer for p in l.ordered_params()], views))
    # with overlap=True the layers are updated exactly once, from inside the second node
    m.zero_grad(set_to_none=True)
    opt = AdamW(m.parameters(), lr=1e-3, model=m, overlap=True)
    calls = []
    inner = opt._early_layer_update
    opt._early_layer_update = lambda li: (calls.append(li), inner(li))[1]
    sink.on_layer_done = opt._sink_hook
    w0 = m.bert.encoder.layer[0].output.dense.weight.detach().clone()
    m.forward_with_cutoff(**batch).loss.backward()
    torch.cuda.synchronize()
    assert sorted(calls) == list(range(len(m.bert.encoder.layer))) and sorted(opt._early) == sorted(calls)
    assert not torch.equal(m.bert.encoder.layer[0].output.dense.weight, w0)
    opt.step()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
def test_accumulating_step_is_deterministic(hip, monkeypatch):
    m, cfg, B, S = _build_mode(hip, "fp32-planes", monkeypatch)
    (a, _), cfgs = _profiled(hip, lambda: _two_micro_batches(m, cfg, B, S, fused=True))
    _check_branch("fp32-planes", cfgs)
    b, _ = _two_micro_batches(m, cfg, B, S, fused=True)
    assert all(torch.equal(a[n], b[n]) for n in a)
