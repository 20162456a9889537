"""Measurements of the tagger's consistency step on one MI355X:

    python tools/consistency_bench.py [--rounds 7] [--steps 8] [--out profiles/consistency_bench.json]

  * kernel: engine.TokenDivergenceFunction forward + backward at 32 x 128 rows of 11 and of 64 tags, both kinds, against the eager
    chain it replaces (log_softmax twice, the two kl_div, autograd) -- device events around 100 back-to-back forward + backward
    pairs per round, the two forms taking turns;
  * step: TVNetSAModel2.forward_consistent + backward + step() at the headline shape (bench.py's model and batch) with
    args.fused_accumulation off and on, against two plain steps (forward + backward + step(), twice) -- host clock around a device
    synchronise, the configurations taking turns.

Reported: the median over the rounds and their min / max.  The default `python bench.py` step against the parent commit is
measured with bench.py itself, the two trees taking turns; its figures are merged into the same file by hand."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
DEV = "cuda:0"


def _stats(xs, unit):
    return {f"median_{unit}": round(statistics.median(xs), 3), f"min_{unit}": round(min(xs), 3), f"max_{unit}": round(max(xs), 3),
            "rounds": len(xs)}


def _eager(x, y, mask, kind):
    lp, lq = F.log_softmax(x, -1), F.log_softmax(y, -1)
    if kind == "sym_kl":
        rows = 0.5 * (F.kl_div(lq, lp, reduction="none", log_target=True) + F.kl_div(lp, lq, reduction="none", log_target=True)).sum(-1)
    else:
        lm = torch.logaddexp(lp, lq) - 0.6931471805599453
        rows = 0.5 * (F.kl_div(lm, lp, reduction="none", log_target=True) + F.kl_div(lm, lq, reduction="none", log_target=True)).sum(-1)
    return (rows * mask).sum() / mask.sum()


def kernel(rounds, reps=100, warmup=20):
    from mtvaf_amd import engine
    res = {}
    lengths = torch.tensor([128 - (7 * i) % 90 for i in range(32)])
    mask = (torch.arange(128)[None, :] < lengths[:, None]).to(DEV)
    maskf = mask.float()
    for C in (11, 64):
        g = torch.Generator().manual_seed(C)
        x = (3 * torch.randn(32, 128, C, generator=g)).to(DEV).requires_grad_(True)
        y = (x.detach() + torch.randn(32, 128, C, generator=g).to(DEV)).requires_grad_(True)
        for kind in ("sym_kl", "js"):
            def run(fn):
                fn().backward()
                x.grad = y.grad = None
            fns = {"kernel": lambda: run(lambda: engine.TokenDivergenceFunction.apply(x, y, mask, kind)),
                   "eager": lambda: run(lambda: _eager(x, y, maskf, kind))}
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
            res[f"32x128x{C}_{kind}"] = {n: _stats(v, "us") for n, v in times.items()}
    res["note"] = "microseconds per forward + backward pair, back to back: includes the host's enqueue cost where it is the longer one"
    return res


def step(rounds, steps, warmup=3):
    import bench
    from mtvaf_amd.optim import AdamW

    def make(fused, overlap):
        model, cfg = bench.build_model(DEV)
        model.train()
        model.args.consistency_weight, model.args.fused_accumulation = 1.0, fused
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model, overlap=overlap)
        ids, mask, tt, labels, feats, aux = bench.synthetic_batch(32, 128, 8, cfg.vocab_size, 1234, DEV)
        return model, opt, dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats,
                                aux_imgs=aux)

    def plain_twice(model, opt, batch):
        def fn():
            for _ in range(2):
                model(**batch).loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
        return fn

    def consistent(model, opt, batch):
        def fn():
            model.forward_consistent(**batch).loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return fn

    # (without the opt-in both encoder nodes take the allocate-and-accumulate fallback and step() updates, as in
    # tools/accumulation_bench.py's cutoff step; with it the layers are updated from inside the second node)
    fns = {"two_plain_steps": plain_twice(*make(False, True)), "consistent": consistent(*make(False, False)),
           "consistent_fused_accumulation": consistent(*make(True, True))}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3 / steps)
    return {n: _stats(v, "ms") for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="kernel,step")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps}
    for part, fn in (("kernel", lambda: kernel(a.rounds)), ("step", lambda: step(a.rounds, a.steps))):
        if part in a.only.split(","):
            res[part] = fn()
            torch.cuda.empty_cache()
            print(json.dumps({part: res[part]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
