"""Measurements of the sharpness-aware step on one MI355X, at the headline shape (bench.py's model:
BERT-base, fp32, batch 32, 128 tokens, 36 prefix slots):

    python tools/sam_bench.py [--steps 24] [--out profiles/sam_bench.json]

  * parts: ``AdamW.perturb()`` alone (norm, finalize, one launch per layer, the multi-tensor rest; the gradients of one backward pass
    are put back before every call), the eager chain it replaces (``torch._foreach_norm`` + ``_foreach_add_`` +
    ``invalidate_weight_images()`` + the image rebuild the next forward pass then pays, measured as that rebuild alone), and the
    restore in both forms (one multi-tensor copy; the forms that rewrite the images).  Device events around every call, median / min /
    max over the rounds.
  * steps: a whole SAM optimizer step (``SharpnessAware.step``) beside the clean step the default configuration takes
    (``AdamW(overlap=True)``) and the clean step of ``AdamW(overlap=False)``; the configurations take turns, every step has its own
    pair of device events."""
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


def _make(overlap, **kw):
    import bench
    from mtvaf_amd.optim import AdamW
    model, cfg = bench.build_model(DEV)
    model.train()
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5, weight_decay=1e-2, model=model, overlap=overlap, **kw)
    ids, mask, tt, labels, feats, aux = bench.synthetic_batch(32, 128, 8, cfg.vocab_size, 1234, DEV)
    batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, imagelabel=None, images=feats, aux_imgs=aux)
    return model, opt, batch


def _timed(fn, prepare, rounds, warmup=3):
    out = []
    for r in range(warmup + rounds):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1), "rounds": len(out)}


def parts(rounds=20, rho=0.05):
    from mtvaf_amd import engine
    m, opt, batch = _make(False, sam_rho=rho)
    m(**batch).loss.backward()  # (also builds the weight images)
    torch.cuda.synchronize()
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    grads = [p.grad for p in params]
    stores = m.bert.encoder._stores
    res = {"parameters": sum(p.numel() for p in params), "image_path": all(st.weights._pl is not None for st in stores)}

    def give_back():  # the first pass's gradients, as perturb() found them (it sets .grad to None; the buffers are the same)
        if opt.sam_perturbed:
            opt.unperturb()
            for st in stores:
                engine._weights_planes(st.weights)
        for p, g in zip(params, grads):
            p.grad = g
        for st in stores:  # (mark the images read, as the forward pass between two steps does)
            if st.weights._pl is not None:
                st.weights._pl[3] = True
        torch.cuda.synchronize()
    res["perturb"] = _timed(opt.perturb, give_back, rounds)
    give_back()

    def eager():
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
        torch._foreach_add_([p.data for p in params], torch._foreach_mul(grads, rho / (norm + 1e-12)))
        engine.invalidate_weight_images()
        for st in stores:  # what the next forward pass then does before its first GEMM
            engine._weights_planes(st.weights)
    backup = [p.detach().clone() for p in params]

    def put_back():
        torch._foreach_copy_([p.data for p in params], backup)
        torch.cuda.synchronize()
    res["eager_chain_with_image_rebuild"] = _timed(eager, put_back, rounds)
    put_back()
    engine.invalidate_weight_images()
    for st in stores:
        engine._weights_planes(st.weights)

    def perturbed():
        give_back()
        opt.perturb()
        for st in stores:
            if st.weights._pl is not None:
                st.weights._pl[3] = True
        torch.cuda.synchronize()
    res["restore_copy"] = _timed(lambda: opt._sam_restore(images=False), perturbed, rounds)
    engine.invalidate_weight_images()
    for st in stores:
        engine._weights_planes(st.weights)
    res["restore_with_images"] = _timed(lambda: opt._sam_restore(images=True), perturbed, rounds)
    return res


def steps(n_steps, warmup=4, rho=0.05):
    from mtvaf_amd.sam import SharpnessAware
    fns = {}
    for name, overlap in (("clean_overlap", True), ("clean_step_after_backward", False)):
        m, o, b = _make(overlap)

        def clean(m=m, o=o, b=b):
            m(**b).loss.backward()
            o.step()
            o.zero_grad(set_to_none=True)
        fns[name] = clean
    m, o, b = _make(False, sam_rho=rho)
    sam = SharpnessAware(m, o)
    fns["sam"] = lambda: sam.step(**b)
    m, o, b = _make(False, sam_rho=rho, max_grad_norm=1.0)
    sam_clip = SharpnessAware(m, o)
    fns["sam_with_clipping"] = lambda: sam_clip.step(**b)
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
    ap.add_argument("--only", default="parts,steps")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    for part, fn in (("parts", parts), ("steps", lambda: steps(a.steps))):
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
