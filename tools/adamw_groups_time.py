"""Times `mtvaf_amd.optim.AdamW.step()` under parameter groups that differ INSIDE an encoder layer (biases and LayerNorm weights
without weight decay: `optim.finetune_param_groups`), and the segmented launch against the uniform one.

    python tools/adamw_groups_time.py [--batch 32 --seq 128 --aux 8 --steps 12 --rounds 5 --launches 20]

1. `step()` of overlap=False on the headline model (BERT-base, fp32 split products, plane images live), three optimizers in one
   process taking turns: the split groups with the segmented plans (one `adamw_planes_seg` launch per layer); the same groups with
   the plans switched off (`SEGMENT_PLANS = False`: the launches of the commit before the segmented path -- every layer tensor
   through `adamw_multi`, then a rebuild of the layer's plane images); and the reference's uniform groups (one `adamw_planes` launch
   per layer) for scale.  The device time of `step()` is taken between two HIP events recorded around it inside whole training steps
   (the plane images are maintained only while forward passes read them), averaged over `--steps` steps; median and range over
   `--rounds` rounds.  With the plans off the stale plane images are rebuilt by the NEXT forward pass, outside `step()`: the whole
   training step (events around all of a round's steps) is reported beside it and is the figure to compare.  Then the first two
   again with overlap=True, where only a layer with a plan is updated from inside the backward pass.
2. One layer's flat buffer (7 087 872 elements, its four matrices' plane images): `adamw_planes` against `adamw_planes_seg` with the
   8-segment table of such a layer, and `adamw` against `adamw_seg` -- the same bytes moved; `--launches` launches back to back
   between two events, the two forms taking turns; median and range over the rounds, and the ratio."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def report(name, xs, unit="ms"):
    print(f"{name:<58s} median {statistics.median(xs):9.4f} {unit}   range {min(xs):9.4f} .. {max(xs):9.4f}   ({len(xs)} rounds)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--aux", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    import bench
    from mtvaf_amd import hip
    from mtvaf_amd.optim import AdamW, finetune_param_groups, reference_param_groups
    dev = "cuda:0"
    hip.set_compute_dtype("fp32")
    ids, mask, tt, labels, feats, aux = bench.synthetic_batch(a.batch, a.seq, a.aux, 30522, 1234, dev)
    kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)

    def make(groups, plans=True, overlap=False):
        model, _ = bench.build_model(dev, "bert", a.seq)
        model.train()
        opt = AdamW(groups(model), lr=3e-5, model=model, overlap=overlap)
        if not plans:
            opt.SEGMENT_PLANS = False
            opt._map_layers()
        return model, opt

    def run(model, opt, steps):
        """-> (ms inside step() on the device, ms of the whole steps)."""
        pairs = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            model(**kw).loss.backward()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            opt.zero_grad(set_to_none=True)
            pairs.append((e0, e1))
        t1.record()
        torch.cuda.synchronize()
        return sum(x.elapsed_time(y) for x, y in pairs) / steps, t0.elapsed_time(t1) / steps

    split = lambda m: finetune_param_groups(m, 3e-5)
    variants = {"split groups, segmented plans": make(split),
                "split groups, plans off (multi-tensor + image rebuild)": make(split, plans=False),
                "uniform groups (reference recipe)": make(lambda m: reference_param_groups(m, 3e-5))}
    kinds = {k: sorted({type(p).__name__ if not isinstance(p, list) else f"{len(p)} segments" for p in o._layer_group.values()})
             for k, (_, o) in variants.items()}
    print(f"BERT-base, bs {a.batch}, S {a.seq}, fp32; {a.steps} steps per round; layer plans: {kinds}", flush=True)
    def compare(variants):
        times, whole = {k: [] for k in variants}, {k: [] for k in variants}
        for m, o in variants.values():
            run(m, o, 3)  # warm-up: workspaces, moments, the weight images
        for _ in range(a.rounds):
            for k, (m, o) in variants.items():
                s, w = run(m, o, a.steps)
                times[k].append(s)
                whole[k].append(w)
        for k in variants:
            report("step(): " + k, times[k])
        for k in variants:
            report("whole training step: " + k, whole[k])
        seg, off = (statistics.median(whole[k]) for k in list(variants)[:2])
        print(f"whole step, segmented - plans off: {seg - off:+.4f} ms ({seg / off:.4f})", flush=True)

    compare(variants)
    del variants
    torch.cuda.empty_cache()
    # the updates inside the backward pass: only a layer with a plan is updated there
    print("overlap=True:", flush=True)
    variants = {"split groups, segmented plans": make(split, overlap=True),
                "split groups, plans off (multi-tensor + image rebuild)": make(split, plans=False, overlap=True)}
    compare(variants)
    del variants
    torch.cuda.empty_cache()

    # -- one layer's buffer: the segmented launch against the uniform one ----------------------------------------------------------
    H, I = 768, 3072
    sizes = [3 * H * H, 3 * H, H * H, 3 * H, I * H, I, H * I, 3 * H]  # wqkv | bqkv | wo | bo ln1 | w1 | bi1 | w2 | bi2 ln2
    ends = [sum(sizes[:i + 1]) for i in range(len(sizes))]
    n = ends[-1]
    table = [(e, 3e-5, 1e-2 if i % 2 == 0 else 0.0) for i, e in enumerate(ends)]
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 0.1
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    mats = [(b, r, c, torch.empty(6 * r * c, dtype=torch.uint8, device=dev))
            for b, r, c in ((0, 3 * H, H), (ends[1], H, H), (ends[3], I, H), (ends[5], H, I))]
    forms = {"adamw_planes (uniform)": lambda t: hip.adamw_planes(p, g, m, v, 3e-5, 0.9, 0.999, 1e-8, 1e-2, t, mats),
             "adamw_planes_seg (8 segments)": lambda t: hip.adamw_planes_seg(p, g, m, v, table, 0.9, 0.999, 1e-8, t, mats),
             "adamw (uniform)": lambda t: hip.adamw(p, g, m, v, 3e-5, 0.9, 0.999, 1e-8, 1e-2, t),
             "adamw_seg (8 segments)": lambda t: hip.adamw_seg(p, g, m, v, table, 0.9, 0.999, 1e-8, t)}

    def burst(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.launches):
            f(t + 1)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches

    for f in forms.values():
        burst(f)
    per = {k: [] for k in forms}
    for _ in range(max(a.rounds, 9)):
        for k, f in forms.items():
            per[k].append(burst(f))
    print(f"one layer's buffer, {n} elements, {a.launches} launches per burst:", flush=True)
    for k in forms:
        report("  " + k, per[k])
    med = {k: statistics.median(x) for k, x in per.items()}
    print(f"planes: segmented / uniform {med['adamw_planes_seg (8 segments)'] / med['adamw_planes (uniform)']:.4f}   "
          f"flat: segmented / uniform {med['adamw_seg (8 segments)'] / med['adamw (uniform)']:.4f}", flush=True)


if __name__ == "__main__":
    main()
