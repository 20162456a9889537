"""Attention probabilities on request (output_attentions) on the MI355X: the kernel against a float64 softmax, the encoder
modules against the reference's golden layer-0 maps and the CPU oracle, and the TVNetSAModel2 switch in the padded and the
padding-free run.

Tolerances are the project's own: the ``close`` rule and the encoder tolerance rtol = 1e-3 of tests/test_model_gpu.py for both
fp32 arithmetics, rtol = 2e-2 (tests/test_ops_gpu.py, bf16 attention forward) for the bf16 compute mode."""
import math
import types

import numpy as np
import pytest
import torch

import params as P
import test_model_gpu as TM
from oracle import mtvaf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
close = TM.close
NH, H, B = 2, 128, 3


# ---------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------
def _op_case(S, Pn):
    """Random Q|K|V rows and prefix keys, ragged lengths (S, 1 and one in between), ONE interior masked key in the full-length
    sentence, and the float64 reference softmax."""
    rng = np.random.default_rng(1000 + 7 * S + Pn)
    qkv = torch.from_numpy(rng.standard_normal((B * S, 3 * H), dtype=np.float32))
    pk = torch.from_numpy(rng.standard_normal((B, max(Pn, 1) * H), dtype=np.float32) * np.float32(0.5))[:, :Pn * H].contiguous()
    lengths = [S, 1, (S + 1) // 2 + 1]
    mask = torch.zeros(B, Pn + S)
    mask[:, :Pn] = 1
    for b, n in enumerate(lengths):
        mask[b, Pn:Pn + n] = 1
    mask[0, Pn + 3] = 0  # a hole: the mask is not only a trailing cut
    addmask = (1.0 - mask) * -10000.0
    q = qkv[:, :H].view(B, S, NH, 64).permute(0, 2, 1, 3).double()
    k = qkv[:, H:2 * H].view(B, S, NH, 64).permute(0, 2, 1, 3).double()
    if Pn:
        k = torch.cat([pk.view(B, NH, Pn, 64).double(), k], 2)
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(64) + addmask[:, None, None, :].double(), -1)
    return qkv, pk, mask, addmask, ref


def _launch(qkv, pk, addmask, S, Pn, zero_masked_queries, want_mass=True):
    from mtvaf_amd import hip
    probs = torch.full((B, NH, S, Pn + S), float("nan"), device=DEV)
    mass = torch.full((B, NH, S), float("nan"), device=DEV) if want_mass else None
    hip.prefix_attn_probs(qkv, pk if Pn else None, addmask, probs, mass, B, S, Pn, NH, zero_masked_queries)
    torch.cuda.synchronize()
    return probs, mass


# one query tile; a prefix; a partial second tile; three tiles with a 2-query remainder; T ending exactly on / just past a key tile
@pytest.mark.parametrize("S,Pn", [(16, 0), (16, 4), (70, 36), (130, 36), (64, 64)])
def test_probs_kernel_matches_float64_softmax(S, Pn, f32_arith):
    qkv, pk, mask, addmask, ref = _op_case(S, Pn)
    qkv_d, pk_d, am_d = qkv.to(DEV), pk.to(DEV), addmask.to(DEV)
    probs, mass = _launch(qkv_d, pk_d, am_d, S, Pn, 0)
    # every element was written (the buffers were NaN before the launch)
    assert not bool(torch.isnan(probs).any()) and not bool(torch.isnan(mass).any())
    got = probs.cpu()
    err = (got.double() - ref).abs()
    print(f"S={S} P={Pn} {f32_arith}: max abs err {float(err.max()):.3e} (ref max {float(ref.max()):.3e}), "
          f"max |rowsum - 1| {float((got.double().sum(-1) - 1).abs().max()):.3e}")
    close(got, ref, rtol=1e-3, name="probs")
    # masked keys (trailing padding and the hole alike) are exactly 0 for every query
    dead = (mask == 0)[:, None, None, :].expand_as(got)
    assert float(got[dead].abs().max()) == 0.0
    # every row is live in this launch and sums to 1
    assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-5
    close(mass.cpu(), got[..., :Pn].double().sum(-1), rtol=1e-3, atol=1e-6 if Pn == 0 else None, name="prefix_mass")
    if Pn == 0:
        assert float(mass.abs().max()) == 0.0
    # two launches are bit-identical
    probs2, mass2 = _launch(qkv_d, pk_d, am_d, S, Pn, 0)
    assert torch.equal(probs, probs2) and torch.equal(mass, mass2)
    # zero_masked_queries: rows whose own key is masked are zeros, the others keep their bits
    pz, mz = _launch(qkv_d, pk_d, am_d, S, Pn, 1)
    assert not bool(torch.isnan(pz).any()) and not bool(torch.isnan(mz).any())
    qdead = (mask[:, Pn:] == 0).to(DEV)  # [B, S]
    rows = qdead[:, None, :].expand(B, NH, S)
    assert bool(qdead.any()) and float(pz[rows].abs().max()) == 0.0 and float(mz[rows].abs().max()) == 0.0
    assert torch.equal(pz[~rows], probs[~rows]) and torch.equal(mz[~rows], mass[~rows])
    # the mass alone (no [B,NH,S,T] stores) carries the same bits
    from mtvaf_amd import hip
    only = torch.full((B, NH, S), float("nan"), device=DEV)
    hip.prefix_attn_probs(qkv_d, pk_d if Pn else None, am_d, None, only, B, S, Pn, NH, 0)
    assert torch.equal(only, mass)
    # and the full maps without the mass
    p3, _ = _launch(qkv_d, pk_d, am_d, S, Pn, 0, want_mass=False)
    assert torch.equal(p3, probs)


# ---------------------------------------------------------------------------------------------------------
# 2. the encoder modules against the reference golden and the CPU oracle
# ---------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_probs(name, cfg):
    """Per-layer probabilities of the CPU oracle fed with its OWN hidden states (computed once per fixture)."""
    if name not in _ORACLE:
        fx = TM.load(name)
        seed, Bf, Pfx = int(fx["seed"]), int(fx["B"]), int(fx["P"])
        sd = P.encoder_params(cfg, seed)
        ids, mask, tt = (torch.from_numpy(fx[k]) for k in ("ids", "mask", "tt"))
        pkv = P.prefix_kv(seed + 2, cfg.layers, Bf, cfg.heads, Pfx)
        full = torch.cat([torch.ones(Bf, Pfx, dtype=mask.dtype), mask], 1) if Pfx else mask
        ohs = O.bert_model(sd, ids, full, tt, pkv, cfg.layers, cfg.heads, cfg.eps, roberta=cfg.roberta, pad_idx=cfg.pad_idx)
        ext = O.extended_attention_mask(full)
        _ORACLE[name] = [O.prefix_self_attention(ohs[i], ext, sd, f"encoder.layer.{i}.attention.self.", cfg.heads,
                                                 pkv[i] if pkv is not None else None, return_probs=True)[1]
                         for i in range(cfg.layers)]
    return _ORACLE[name]


def _golden_model(name, cfg):
    fx = TM.load(name)
    seed, Bf, Pfx = int(fx["seed"]), int(fx["B"]), int(fx["P"])
    m = TM.build_encoder(cfg)
    missing, unexpected = m.load_state_dict(P.encoder_params(cfg, seed), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    m.to(DEV).eval()
    ids, mask, tt = (torch.from_numpy(fx[k]).to(DEV) for k in ("ids", "mask", "tt"))
    pkv = P.prefix_kv(seed + 2, cfg.layers, Bf, cfg.heads, Pfx)
    if pkv is not None:
        pkv = [(k.to(DEV), v.to(DEV)) for k, v in pkv]
    full = torch.cat([torch.ones(Bf, Pfx, dtype=mask.dtype, device=DEV), mask], 1) if Pfx else mask
    return fx, m, dict(input_ids=ids, attention_mask=full, token_type_ids=tt, past_key_values=pkv)


GOLDEN = [("enc_tiny_bert_P0", P.TINY_BERT), ("enc_tiny_bert_P4", P.TINY_BERT), ("enc_tiny_bert_P16", P.TINY_BERT),
          ("enc_tiny_bert_P36", P.TINY_BERT), ("enc_tiny_roberta_P4", P.TINY_ROBERTA)]


@pytest.mark.parametrize("name,cfg", GOLDEN)
def test_encoder_attentions_match_reference_golden(name, cfg, f32_arith):
    fx, m, kw = _golden_model(name, cfg)
    Bf, S, Pfx = int(fx["B"]), int(fx["S"]), int(fx["P"])
    out = m(output_attentions=True, output_hidden_states=True, return_dict=True, **kw)
    att = out["attentions"]
    assert att is not None and len(att) == cfg.layers
    for a in att:
        assert tuple(a.shape) == (Bf, cfg.heads, S, Pfx + S) and a.dtype == torch.float32 and not a.requires_grad
    close(att[0], fx["attn_l0"], rtol=1e-3, name="attentions[0] vs the reference")
    for i, ref in enumerate(_oracle_probs(name, cfg)):
        close(att[i], ref, rtol=1e-3, name=f"attentions[{i}] vs the oracle")
    # a selection of layers: same length, None elsewhere, the same bits
    sel = m(output_attentions=[1], return_dict=True, **kw)["attentions"]
    assert isinstance(sel, tuple) and len(sel) == cfg.layers and sel[0] is None and torch.equal(sel[1], att[1])
    # nothing requested: nothing returned
    assert m(return_dict=True, **kw).attentions is None
    assert m(output_attentions=False, return_dict=True, **kw).attentions is None
    # the tuple form carries them last
    tup = m(output_attentions=True, output_hidden_states=True, return_dict=False, **kw)
    assert len(tup) == 4 and torch.equal(tup[3][0], att[0])


def test_encoder_attentions_in_training_mode_leave_the_gradients_alone():
    """train(): the maps are the probabilities before dropout, detached; the backward pass of the same forward gives the
    gradients it gives without them."""
    name, cfg = GOLDEN[1]
    fx, m, kw = _golden_model(name, cfg)
    m.train()
    gw = torch.from_numpy(fx["grad_seed_w"]).to(DEV)
    grads = []
    for flag in (False, True):
        m.zero_grad(set_to_none=True)
        out = m(output_attentions=flag, return_dict=True, **kw)
        (out["last_hidden_state"] * gw).sum().backward()
        grads.append(m.encoder.layer[0].attention.self.query.weight.grad.clone())
        if flag:
            close(out["attentions"][0], fx["attn_l0"], rtol=1e-3, name="attentions[0], train mode")
    assert torch.equal(grads[0], grads[1])


def test_attention_maps_in_bf16_compute_mode():
    """hip.COMPUTE = "bf16": the Q|K projection rounds its operands to bf16 (the process's compute mode); the bar is the one of
    the bf16 attention forward."""
    from mtvaf_amd import engine, hip
    name, cfg = GOLDEN[2]
    fx, m, kw = _golden_model(name, cfg)
    was = hip.COMPUTE
    hip.set_compute_dtype("bf16")
    try:
        att = m(output_attentions=True, return_dict=True, **kw)["attentions"]
    finally:
        hip.set_compute_dtype(was)
    for i, ref in enumerate(_oracle_probs(name, cfg)):
        err = (att[i].cpu() - ref).abs().max()
        print(f"bf16 layer {i}: max abs err {float(err):.3e} (ref max {float(ref.max()):.3e})")
        close(att[i], ref, rtol=2e-2, name=f"attentions[{i}], bf16 compute")


# ---------------------------------------------------------------------------------------------------------
# 3. the drop-in model
# ---------------------------------------------------------------------------------------------------------
def test_tvnet2_attentions_switch_padded_and_padding_free(f32_arith):
    from mtvaf_amd import engine
    cfg = P.EncCfg(vocab_size=500, hidden=768, heads=12, inter=128, layers=2, max_pos=64)
    Bm, S, n_aux = 16, 32, 3
    Pn = 4 * (1 + n_aux)
    seed = 40
    args = TM.make_args()
    m = TM.build_tvnet2(cfg, args, sde=P.encoder_params(cfg, seed, std=0.03), sdh=P.head_params(cfg, seed + 10),
                        sdp=P.prompt_params(seed + 20, layers=cfg.layers))
    m.eval()
    # 192 of 512 token rows are unmasked: the padding-free run packs them into 256 rows (it needs a whole 128-row tile to gain)
    lengths = [32, 9, 17, 5, 12, 24, 3, 8, 16, 11, 6, 20, 4, 13, 10, 2]
    ids, mask, tt, labels = P.text_batch(cfg, seed + 1, Bm, S, lengths=lengths, lo_id=5)
    feats, aux, lab = TM._prompt_inputs(seed + 2, Bm, n_aux)
    kw = dict(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), token_type_ids=tt.to(DEV), labels=labels.to(DEV),
              imagelabel=lab.to(DEV), images=feats.to(DEV), aux_imgs=aux.to(DEV))
    assert not hasattr(args, "output_attentions")
    with engine.padding_free(True):
        plain = m(**kw)
        assert engine.LAST_PACK is not None, "the batch must be one that the padding-free run packs"
        assert plain.attentions is None and m.last_prefix_mass is None
        args.output_attentions = True
        args.output_prefix_mass = True
        free = m(**kw)
        free_mass = m.last_prefix_mass
        assert engine.LAST_PACK is not None
    with engine.padding_free(False):
        padded = m(**kw)
        padded_mass = m.last_prefix_mass
        assert engine.LAST_PACK is None
    torch.cuda.synchronize()
    # the switch changes nothing else
    assert float(free.loss) == float(plain.loss) and list(free.logits) == list(plain.logits)
    assert len(free.attentions) == len(padded.attentions) == cfg.layers
    live = mask.bool().to(DEV)[:, None, :].expand(Bm, cfg.heads, S)  # [B, NH, S]: queries whose own key is unmasked
    assert bool((~live).any())
    for i in range(cfg.layers):
        a, b = free.attentions[i], padded.attentions[i]
        assert tuple(a.shape) == tuple(b.shape) == (Bm, cfg.heads, S, Pn + S)
        close(a[live], b[live], rtol=1e-3, name=f"layer {i}: unmasked queries, padding-free vs padded")
        assert float(a[~live].abs().max()) == 0.0
        assert float((b.double().sum(-1) - 1).abs().max()) <= 1e-5  # the padded run computes every row, as the reference
    # the prefix mass alone: [L, B, NH, S], the same figure as the sum over the maps' prefix columns
    assert tuple(free_mass.shape) == tuple(padded_mass.shape) == (cfg.layers, Bm, cfg.heads, S)
    for i in range(cfg.layers):
        close(padded_mass[i], padded.attentions[i][..., :Pn].double().sum(-1), rtol=1e-3, name=f"layer {i}: prefix mass")
        close(free_mass[i][live], padded_mass[i][live], rtol=1e-3, name=f"layer {i}: prefix mass, padding-free vs padded")
    # mass without maps
    args.output_attentions = False
    with engine.padding_free(False):
        only = m(**kw)
        assert only.attentions is None and torch.equal(m.last_prefix_mass, padded_mass)
