"""Measurements of the adversarial step on one MI355X:

    python tools/adversarial_bench.py [--steps 24] [--out profiles/adversarial_bench.json]

  * mtvaf_adv_perturb alone at the headline shape (32 x 128 x 768, bench.py's ragged lengths): FGM and one PGD step (L2, sentence
    scope), and the eager-torch chain of the same arithmetic; device events around `reps` back-to-back calls, median of the rounds;
  * a whole optimizer step of the headline model (bench.py's: BERT-base, fp32, batch 32, 128 tokens, 36 prefix slots): clean
    (AdamW(overlap=True), the default step), FGM on the fallback (AdamW(overlap=False)), FGM with AdamW(overlap=True,
    accumulation_steps=2), and FGM on the fallback with the perturbation made by the eager-torch chain.  The configurations take
    turns; every step is timed by its own pair of device events; reported: median, min and max over `steps` steps after warm-up."""
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


def eager_fgm(g, mask, eps):
    """The chain of torch ops the kernel replaces (L2, sentence scope, no delta_in): double sum of squares, the degenerate units
    by a mask instead of a host read-back -> (delta, stats)."""
    live = mask.ne(0)[..., None]
    gl = torch.where(live, g, torch.zeros((), device=g.device))
    n = gl.double().pow(2).sum((1, 2)).sqrt().float()
    ok = torch.isfinite(n) & (n > 0)
    delta = torch.where(ok[:, None, None], eps * (gl / torch.where(ok, n, torch.ones_like(n))[:, None, None]), torch.zeros((), device=g.device))
    return delta, torch.stack([n, delta.double().pow(2).sum((1, 2)).sqrt().float()], 1)


def eager_pgd(g, mask, delta_in, eps, step):
    live = mask.ne(0)[..., None]
    zero = torch.zeros((), device=g.device)
    gl = torch.where(live, g, zero)
    n = gl.double().pow(2).sum((1, 2)).sqrt().float()
    ok = torch.isfinite(n) & (n > 0)
    d = torch.where(live, delta_in, zero) + step * torch.where(ok[:, None, None], gl / torch.where(ok, n, torch.ones_like(n))[:, None, None], zero)
    nd = d.double().pow(2).sum((1, 2)).sqrt().float()
    d = torch.where((nd > eps)[:, None, None], d * (eps / nd.clamp_min(1e-30))[:, None, None], d)
    return d, torch.stack([n, d.double().pow(2).sum((1, 2)).sqrt().float()], 1)


def _events(fns, rounds, reps, warmup=20):
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
                "calls_per_round": reps} for n, v in times.items()}


def kernel(rounds=20, reps=100):
    import bench
    from mtvaf_amd import hip
    B, S, H = 32, 128, 768
    mask = bench.synthetic_batch(B, S, 8, 30522, 1234, DEV)[1]
    gen = torch.Generator().manual_seed(0)
    g = (torch.randn(B, S, H, generator=gen) * 1e-6).to(DEV)
    din = (torch.randn(B, S, H, generator=gen) * 1e-2).to(DEV)
    x = torch.randn(B, S, H, generator=gen).to(DEV)
    m8 = hip.adv_mask(mask)
    d, o, st = torch.empty_like(g), torch.empty_like(g), torch.empty(B, 2, device=DEV)
    fns = {"fgm_kernel": lambda: hip.adv_perturb(g, m8, 1.0, delta_out=d, stats=st),
           "pgd_step_kernel": lambda: hip.adv_perturb(g, m8, 1.0, 0.5, delta_in=din, delta_out=d, stats=st),
           "fgm_kernel_with_out": lambda: hip.adv_perturb(g, m8, 1.0, x=x, delta_out=d, out=o, stats=st),
           "fgm_eager_torch": lambda: eager_fgm(g, mask, 1.0),
           "pgd_step_eager_torch": lambda: eager_pgd(g, mask, din, 1.0, 0.5)}
    res = _events(fns, rounds, reps)
    res["bytes_read_written_fgm"] = int(mask.ne(0).sum()) * H * 4 * 2 + B * S * H * 4  # g twice over the live rows, delta once
    return res


def steps(n_steps, warmup=4):
    import bench
    from mtvaf_amd import engine, hip
    from mtvaf_amd.adversarial import Adversary
    from mtvaf_amd.optim import AdamW

    def make(overlap, k):
        model, cfg = bench.build_model(DEV)
        model.train()
        kw = {"accumulation_steps": k} if k > 1 else {}
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model, overlap=overlap, **kw)
        return model, cfg, opt

    def batch_of(cfg):
        ids, mask, tt, labels, feats, aux = bench.synthetic_batch(32, 128, 8, cfg.vocab_size, 1234, DEV)
        return dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)

    fns = {}
    m, cfg, o = make(True, 1)
    b = batch_of(cfg)

    def clean(m=m, o=o, b=b):
        m(**b).loss.backward()
        o.step()
        o.zero_grad(set_to_none=True)
    fns["clean"] = clean

    def adv_stepper(overlap, k):
        m, cfg, o = make(overlap, k)
        adv, b = Adversary(m, eps=1.0, optimizer=o), batch_of(cfg)

        def step():
            adv.step(**b)
            o.step()
            o.zero_grad(set_to_none=True)
        return step
    fns["fgm_fallback"] = adv_stepper(False, 1)
    fns["fgm_fused_accumulation"] = adv_stepper(True, 2)

    m, cfg, o = make(False, 1)
    b = batch_of(cfg)

    def eager(m=m, o=o, b=b):  # Adversary.step's passes with the eager chain in the kernel's place
        tap = engine.EmbeddingTap(capture=True)
        m.bert.embedding_tap = tap
        try:
            m(**b).loss.backward()
            tap.delta, tap.capture = eager_fgm(tap.grad.contiguous(), b["attention_mask"], 1.0)[0], False
            m(**b).loss.backward()
        finally:
            m.bert.embedding_tap = None
        o.step()
        o.zero_grad(set_to_none=True)
    fns["fgm_fallback_eager_delta"] = eager

    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(n_steps):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1))
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "steps": len(v)}
            for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="kernel,steps")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    for part, fn in (("kernel", kernel), ("steps", lambda: steps(a.steps))):
        if part not in a.only.split(","):
            continue
        res[part] = fn()
        print(json.dumps({part: res[part]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
