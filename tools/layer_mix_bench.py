"""Measurements of the layer mix on one MI355X:

    python tools/layer_mix_bench.py [--rounds 10] [--reps 50] [--steps 30] [--out profiles/layer_mix_bench.json]

1. The mix alone at the headline shape (32 x 128 x 768, K = 13): forward + backward of the kernels (mtvaf_layer_mix_fwd, _dots and
   the 13 injections into one running gradient) against the eager padded chain they replace (stack, softmax, weighted sum,
   autograd down to the 13 hidden-state gradients and their sum).  The two take turns; device events around `reps` back-to-back
   calls; reported: median, min and max over the rounds.
2. The headline training step (bench.py's model, batch and optimizer) with args.layer_mix = "all" against the same step
   without: two models, alternating rounds of `steps` steps, device events per round.
The default step against the parent commit is bench.py's own figure, taken in both trees in one session."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
DEV = "cuda:0"


def _stats(v, unit):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), f"max_{unit}": round(max(v), 3),
            "rounds": len(v)}


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def mix_alone(rounds, reps, warmup=10):
    from mtvaf_amd import hip
    B, S, H, K = 32, 128, 768, 13
    gen = torch.Generator().manual_seed(0)
    states = [torch.randn(B, S, H, generator=gen).to(DEV) for _ in range(K)]
    dy = torch.randn(B, S, H, generator=gen).to(DEV)
    a = torch.randn(K, generator=gen).to(DEV).requires_grad_(True)
    g = torch.full((1,), 0.7, device=DEV).requires_grad_(True)
    leaves = [h.clone().requires_grad_(True) for h in states]

    def kernels():
        hip.layer_mix_fwd(states, a.detach(), g.detach())
        _, _, coef = hip.layer_mix_dots(states, dy, a.detach(), g.detach())
        dh = None
        for j in range(K - 1, -1, -1):  # (the encoder backward meets the states top down)
            dh = hip.layer_mix_inject(coef, j, dy, dh)
        return dh

    def eager():
        s = torch.softmax(a, 0)
        y = g * (torch.stack(leaves) * s.view(-1, 1, 1, 1)).sum(0)
        y.backward(dy)
        dh = leaves[-1].grad
        for h in reversed(leaves[:-1]):  # (what the encoder's node does with K incoming gradient tensors)
            dh = dh + h.grad
        for t in leaves + [a, g]:
            t.grad = None
        return dh

    x, z = kernels(), eager()
    assert float((x - z).abs().max()) <= 1e-5 * float(z.abs().max())
    fns = {"fwd_bwd_kernels": kernels, "fwd_bwd_eager_torch": eager}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(_timed(fn, reps) * 1e3)
    return {n: dict(_stats(v, "us"), calls_per_round=reps) for n, v in times.items()}


def headline_step(rounds, steps, warmup=8):
    import bench
    from mtvaf_amd.modules.layer_mix import LayerMix
    from mtvaf_amd.optim import AdamW
    B, S = 32, 128
    runs = {}
    for name in ("option_off", "option_on"):
        model, cfg = bench.build_model(DEV)
        if name == "option_on":
            model.layer_mix = LayerMix(cfg.num_hidden_layers + 1).to(DEV)
        model.train()
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model, overlap=True)
        ids, mask, tt, labels, feats, aux = bench.synthetic_batch(B, S, 8, cfg.vocab_size, 1234, DEV)

        def step(model=model, opt=opt):
            out = model(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats,
                        aux_imgs=aux)
            out.loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            assert len(out.logits) == B
        runs[name] = step
    for step in runs.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(rounds):
        for n, step in runs.items():
            times[n].append(_timed(step, steps))
    return {n: dict(_stats(v, "ms"), steps_per_round=steps) for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "mix_alone_32x128x768_K13": mix_alone(a.rounds, a.reps),
           "headline_step": headline_step(a.rounds, a.steps)}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
