"""Measurements of the token cross entropy on one MI355X:

    python tools/token_ce_bench.py [--rounds 7] [--steps 8] [--out profiles/token_ce_bench.json]

  * kernel: modules.token_head.TokenCrossEntropy forward + backward at 32 x 128 rows of 11 and of 64 tags -- plain, and with class
    weights, smoothing 0.1 and focal gamma 2 -- against the eager chain it replaces (log_softmax, gather, the weighted and
    smoothed sums, where, autograd) -- device events around 100 back-to-back forward + backward pairs per round, the two forms
    taking turns;
  * step: the headline step (bench.py's model and batch: forward + backward + step()) with args.token_ce_weight 0 (the default:
    nothing is launched for the term) and 0.5 -- host clock around a device synchronise, the configurations taking turns.

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


def _eager(z, labels, live, weight, smoothing, gamma, B):
    """The batch-mean loss as torch ops: the chain a user writes without the kernels."""
    C = z.shape[-1]
    lp = F.log_softmax(z, -1)
    y = torch.where(live, labels, torch.zeros_like(labels))
    lpy = lp.gather(-1, y[..., None])[..., 0]
    if weight is None:
        ce = -(1.0 - smoothing) * lpy - (smoothing / C) * lp.sum(-1) if smoothing else -lpy
    else:
        ce = -(1.0 - smoothing) * weight[y] * lpy
        if smoothing:
            ce = ce - (smoothing / C) * (lp * weight).sum(-1)
    if gamma:
        ce = (1.0 - lpy.exp()).clamp_min(0).pow(gamma) * ce
    return torch.where(live, ce, torch.zeros_like(ce)).sum() / B


def kernel(rounds, reps=100, warmup=20):
    from mtvaf_amd.modules.token_head import TokenCrossEntropy
    res = {}
    B, S = 32, 128
    lengths = torch.tensor([S - (7 * i) % 90 for i in range(B)])
    mask = (torch.arange(S)[None, :] < lengths[:, None]).to(DEV)
    mask_u8 = mask.to(torch.uint8)
    for C in (11, 64):
        g = torch.Generator().manual_seed(C)
        z = (3 * torch.randn(B, S, C, generator=g)).to(DEV).requires_grad_(True)
        labels = torch.randint(0, C, (B, S), generator=g).to(DEV)
        wts = (0.1 + torch.rand(C, generator=g)).to(DEV)
        for name, weight, smoothing, gamma in (("plain", None, 0.0, 0.0), ("weighted_smoothed_focal", wts, 0.1, 2.0)):
            head = TokenCrossEntropy(C, None if weight is None else weight.tolist(), smoothing, gamma).to(DEV)

            def run(fn):
                fn().backward()
                z.grad = None
            fns = {"kernel": lambda: run(lambda: head(z, labels, mask_u8, "batch_mean")),
                   "eager": lambda: run(lambda: _eager(z, labels, mask, weight, smoothing, gamma, B))}
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
            res[f"{B}x{S}x{C}_{name}"] = {n: _stats(v, "us") for n, v in times.items()}
    res["note"] = "microseconds per forward + backward pair, back to back: includes the host's enqueue cost where it is the longer one"
    return res


def step(rounds, steps, warmup=3):
    import bench
    from mtvaf_amd.optim import AdamW

    def make(weight):
        import mtvaf_amd.models.bert_model as bm
        model, cfg = bench.build_model(DEV)
        if weight:  # (the options are read at construction: the head is built here as the constructor would)
            model.args.token_ce_weight = weight
            model.token_opt = bm._token_head_options(model.args, model.num_labels)
            from mtvaf_amd.modules.token_head import TokenCrossEntropy
            model.token_ce = TokenCrossEntropy(model.num_labels).to(DEV)
        model.train()
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model)
        ids, mask, tt, labels, feats, aux = bench.synthetic_batch(32, 128, 8, cfg.vocab_size, 1234, DEV)
        batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)

        def fn():
            model(**batch).loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return fn

    fns = {"default": make(0.0), "token_ce_weight_0.5": make(0.5)}
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
