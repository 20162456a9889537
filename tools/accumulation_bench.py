"""Measurements of the fused gradient accumulation on one MI355X:

    python tools/accumulation_bench.py [--rounds 5] [--steps 8] [--out profiles/accumulation_bench.json]

  * time per OPTIMIZER step of the headline model (bench.py's: BERT-base, 128 tokens, 36 prefix slots) as one batch of 32 (the
    default step, accumulation off) and as two micro-batches of 16 with the fallback (overlap=False) and fused
    (AdamW(overlap=True, accumulation_steps=2));
  * the cutoff step (TVNetSAModel.forward_with_cutoff + backward + step) with args.fused_accumulation off and on;
  * the grouped pre-split weight-gradient launch at the headline layer shape, overwriting against accumulating (device events around
    200 back-to-back launches).

Every configuration is warmed up, then the configurations take turns for `rounds` rounds of `steps` steps (host clock around a device
synchronise); reported: the median of the rounds' per-step means and their min / max.  On a tree without the feature the fused
configurations are reported as absent, so the same script measures the parent commit."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
DEV = "cuda:0"


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "rounds": len(xs)}


def _take_turns(steps_by_name, rounds, steps, warmup=3):
    for fn in steps_by_name.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in steps_by_name}
    for _ in range(rounds):
        for n, fn in steps_by_name.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3 / steps)
    return {n: _stats(v) for n, v in times.items()}


def headline(rounds, steps):
    import bench
    from mtvaf_amd.optim import AdamW
    fused_ok = "accumulation_steps" in AdamW.__init__.__code__.co_varnames

    def make(overlap, k):
        model, cfg = bench.build_model(DEV)
        model.train()
        kw = {"accumulation_steps": k} if (k > 1 and overlap) else {}
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model, overlap=overlap, **kw)
        return model, cfg, opt

    def stepper(model, opt, batches):
        def step():
            for ids, mask, tt, labels, feats, aux in batches:
                out = model(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)
                (out.loss / len(batches)).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return step

    fns = {}
    m, cfg, o = make(True, 1)
    fns["default_batch32"] = stepper(m, o, [bench.synthetic_batch(32, 128, 8, cfg.vocab_size, 1234, DEV)])
    micro = [bench.synthetic_batch(16, 128, 8, cfg.vocab_size, 1234 + i, DEV) for i in range(2)]
    m, cfg, o = make(False, 2)
    fns["accum2_fallback"] = stepper(m, o, micro)
    if fused_ok:
        m, cfg, o = make(True, 2)
        fns["accum2_fused"] = stepper(m, o, micro)
    res = _take_turns(fns, rounds, steps)
    if not fused_ok:
        res["accum2_fused"] = None
    return res


def cutoff(rounds, steps):
    import params as P
    from test_model_gpu import LABELS, _prompt_inputs, hf_config, make_args
    from mtvaf_amd.models.bert_model import TVNetSAModel
    from mtvaf_amd.optim import AdamW
    cfg = P.EncCfg(vocab_size=30522, hidden=768, heads=12, inter=3072, layers=12, max_pos=128)
    B, S, M = 16, 128, 8
    lengths = [S - (7 * i) % 90 for i in range(B)]
    ids, mask, tt, _ = P.text_batch(cfg, 3, B, S, lengths, lo_id=5)
    starts, ends, spos, epos, pol, lm = P.span_batch(cfg, 4, B, S, M, lengths)
    feats, aux, _ = _prompt_inputs(11, B, 2)
    batch = {k: v.to(DEV) for k, v in dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, start_positions=spos, end_positions=epos,
                                            span_starts=starts, span_ends=ends, polarity_labels=pol, label_masks=lm, images=feats,
                                            aux_imgs=aux).items()}
    fns = {}
    for name, fused in (("cutoff_fallback", False), ("cutoff_fused", True)):
        args = make_args(use_prefix=True, gcn_layer_number=0, num_layers=0, aug_type="span_cutoff", aug_cutoff_ratio=0.3)
        args.bert_config = hf_config(cfg, dropout=0.1)
        args.fused_accumulation = fused
        torch.manual_seed(0)
        m = TVNetSAModel(LABELS, None, args).to(DEV).train()
        # (fallback: the tree's behaviour without the opt-in, where build_optimizer's overlap never gets a flat buffer and step() updates)
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=3e-5, model=m, overlap=fused)

        def step(m=m, opt=opt):
            m.forward_with_cutoff(**batch).loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        fns[name] = step
    return _take_turns(fns, rounds, steps)


def _take_turns_events(fns, rounds, reps, warmup=20):
    """Device-event timing of `reps` back-to-back launches per round (the host only enqueues: its clock and the launch gaps of a
    synchronised loop are not in the figure) -> per-launch microseconds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {n: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "rounds": len(v),
                "launches_per_round": reps} for n, v in times.items()}


def kernel(rounds, reps=200):
    from mtvaf_amd import hip
    if "accumulate" not in hip.gemm_planes_dw_group.__code__.co_varnames:
        return None
    K, H, I = 2432, 768, 3072  # the packed token rows of the headline batch, BERT-base
    g = torch.Generator().manual_seed(0)
    shapes = [(H, I), (I, H), (H, H), (3 * H, H)]
    pas = [hip.Planes(torch.randn(K, M, generator=g).to(DEV), True) for M, _ in shapes]
    pbs = [hip.Planes(torch.randn(K, N, generator=g).to(DEV), True) for _, N in shapes]
    outs = [torch.zeros(M, N, device=DEV) for M, N in shapes]
    items = list(zip(pas, pbs, outs))
    fns = {"dw_group_overwrite": lambda: hip.gemm_planes_dw_group(items), "dw_group_accumulate": lambda: hip.gemm_planes_dw_group(items, accumulate=True)}
    res = _take_turns_events(fns, max(rounds, 7), reps)
    res["c_bytes_read_extra"] = sum(M * N * 4 for M, N in shapes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="headline,cutoff,kernel")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps}
    for part, fn in (("headline", lambda: headline(a.rounds, a.steps)), ("cutoff", lambda: cutoff(a.rounds, a.steps)),
                     ("kernel", lambda: kernel(a.rounds))):
        if part not in a.only.split(","):
            continue
        try:
            res[part] = fn()
        except Exception as e:  # a part that cannot run on this tree is reported, the others are still measured
            res[part] = {"error": f"{type(e).__name__}: {e}"}
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        print(json.dumps({part: res[part]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
