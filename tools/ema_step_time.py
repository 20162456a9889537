"""Times what the averaged weights (EMA) of `mtvaf_amd.optim.AdamW` cost on the headline model (BERT-base, bs 32, S 128).

    python tools/ema_step_time.py [--batch 32 --seq 128 --aux 8 --steps 12 --rounds 5 --dtype fp32]

`step()` of overlap=False in three variants, in one process, on one model: ema_decay = 0; the fused average (ema_decay = 0.999);
ema_decay = 0 followed by `torch._foreach_lerp_` over the same tensors (the average as a pass of its own).  The device time of
`step()` (+ the lerp) is taken between two HIP events recorded around it inside whole training steps -- the plane images an update
maintains exist only while forward passes read them, so back-to-back `step()` calls alone would time another form of the update --
and summed over `--steps` steps; the variants take turns for `--rounds` rounds, and each is reported as median and range over the
rounds.  Then the whole step with overlap=True (the per-layer updates run inside the backward pass), average off and on, in
sentences/s."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--aux", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    a = ap.parse_args()
    import bench
    from mtvaf_amd import hip
    from mtvaf_amd.optim import AdamW
    dev = "cuda:0"
    hip.set_compute_dtype(a.dtype)
    ids, mask, tt, labels, feats, aux = bench.synthetic_batch(a.batch, a.seq, a.aux, 30522, 1234, dev)
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)

    def make(overlap, decay):
        model, _ = bench.build_model(dev, "bert", a.seq)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        return model, AdamW(params, lr=3e-5, weight_decay=1e-2, model=model, overlap=overlap, ema_decay=decay), params

    def run(model, opt, steps, after=None):
        """-> (ms inside step() [+ after()] on the device, ms of the whole steps)."""
        pairs = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            model(**kw).loss.backward()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            if after is not None:
                after()
            e1.record()
            opt.zero_grad(set_to_none=True)
            pairs.append((e0, e1))
        t1.record()
        torch.cuda.synchronize()
        return sum(x.elapsed_time(y) for x, y in pairs) / steps, t0.elapsed_time(t1) / steps

    def report(name, xs, unit="ms"):
        print(f"{name:<44s} median {statistics.median(xs):9.3f} {unit}   range {min(xs):9.3f} .. {max(xs):9.3f}   ({len(xs)} rounds)", flush=True)

    # -- step() after the backward pass -------------------------------------------------------------------------------------
    variants = {}
    m0, o0, p0 = make(False, 0.0)
    variants["ema_decay = 0"] = (m0, o0, None)
    m1, o1, _ = make(False, a.decay)
    variants["fused average"] = (m1, o1, None)
    m2, o2, p2 = make(False, 0.0)
    shadow = [torch.zeros_like(p) for p in p2]
    variants["ema_decay = 0, then torch._foreach_lerp_"] = (m2, o2, lambda: torch._foreach_lerp_(shadow, [p.detach() for p in p2], 1.0 - a.decay))
    n_params = sum(p.numel() for p in p0)
    print(f"BERT-base, bs {a.batch}, S {a.seq}, {a.dtype}: {n_params / 1e6:.1f} M trained parameters; {a.steps} steps per round", flush=True)
    times = {k: [] for k in variants}
    for k, (m, o, after) in variants.items():
        run(m, o, 3, after)  # warm-up: workspaces, the averages, the weight images
    for _ in range(a.rounds):
        for k, (m, o, after) in variants.items():
            times[k].append(run(m, o, a.steps, after)[0])
    for k in variants:
        report("step(), overlap=False: " + k if k == "ema_decay = 0" else "  " + k, times[k])
    base = statistics.median(times["ema_decay = 0"])
    print(f"fused / plain {statistics.median(times['fused average']) / base:.3f} (bytes alone: {36 / 28:.3f}); "
          f"unfused / plain {statistics.median(times['ema_decay = 0, then torch._foreach_lerp_']) / base:.3f} (bytes alone: {40 / 28:.3f})", flush=True)
    del variants, m0, o0, m1, o1, m2, o2, shadow
    torch.cuda.empty_cache()

    # -- the whole step with the updates inside the backward pass -----------------------------------------------------------
    full = {"overlap=True, ema_decay = 0": make(True, 0.0), "overlap=True, fused average": make(True, a.decay)}
    rates = {k: [] for k in full}
    for k, (m, o, _) in full.items():
        run(m, o, 3)
    for _ in range(a.rounds):
        for k, (m, o, _) in full.items():
            rates[k].append(a.batch / (run(m, o, a.steps)[1] * 1e-3))
    for k in full:
        report(k, rates[k], "sentences/s")


if __name__ == "__main__":
    main()
