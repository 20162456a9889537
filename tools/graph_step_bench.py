"""Step time of the whole-step graph with the optimizer inside against the arrangement it replaces.

    python tools/graph_step_bench.py [--batch 4 --seq 64 --aux 3 --dtype fp32 --steps 40 --warmup 5 --rounds 5 --out FILE.json]

Two arrangements of the same training step (bench.py's model and synthetic batch, train mode), built and timed alternately in one
process, `rounds` times each:
  eager_opt   GraphedTrainStep(model, batch) + AdamW(overlap=False).step() + LambdaLR.step() + zero_grad   (one replay, then the
              Python walk over every parameter and ~20 eager launches)
  graphed_opt GraphedTrainStep(model, batch, optimizer=AdamW(device_schedule=...)) + zero_grad           (one replay, host counters)
A round's figure is wall time / steps between two synchronisations; the line printed last holds both medians, their spreads
(min .. max over the rounds) and the difference."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def one_round(arrangement, args, device):
    import bench
    from mtvaf_amd import hip
    from mtvaf_amd.graph import GraphedTrainStep
    from mtvaf_amd.optim import AdamW, linear_warmup_factor, schedule_table
    hip.set_compute_dtype(args.dtype)
    try:
        model, cfg = bench.build_model(device, "bert", args.seq)
        model.train()
        ids, mask, tt, labels, feats, aux = bench.synthetic_batch(args.batch, args.seq, args.aux, cfg.vocab_size, 1234, device)
        kw = dict(input_ids=ids, attention_mask=mask, token_type_ids=tt, labels=labels, images=feats, aux_imgs=aux)
        params = [p for p in model.parameters() if p.requires_grad]
        total = args.warmup + args.steps
        factor = linear_warmup_factor(0.01 * total, total)
        if arrangement == "graphed_opt":
            opt = AdamW(params, lr=3e-5, weight_decay=1e-2, model=model, overlap=False, device_schedule=schedule_table(factor, total))
            gstep = GraphedTrainStep(model, kw, optimizer=opt)

            def step():
                out = gstep(**kw)
                opt.zero_grad(set_to_none=True)
                return out
        else:
            opt = AdamW(params, lr=3e-5, weight_decay=1e-2, model=model, overlap=False)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, factor)
            gstep = GraphedTrainStep(model, kw)

            def step():
                out = gstep(**kw)
                opt.step()
                sched.step()
                opt.zero_grad(set_to_none=True)
                return out
        try:
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            gc.collect()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = step()
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            loss = float(out.loss)
        finally:
            gstep.close()
        return ms, loss
    finally:
        hip.set_compute_dtype("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=64)
    ap.add_argument("--aux", type=int, default=3)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = "cuda:0"
    times = {"eager_opt": [], "graphed_opt": []}
    losses = {}
    for r in range(args.rounds):
        for arrangement in ("eager_opt", "graphed_opt") if r % 2 == 0 else ("graphed_opt", "eager_opt"):
            ms, loss = one_round(arrangement, args, device)
            times[arrangement].append(round(ms, 4))
            losses[arrangement] = round(loss, 4)
            print(f"[graph_step_bench] round {r} {arrangement}: {ms:.3f} ms/step, loss {loss:.4f}", flush=True)
    res = {"config": f"bs {args.batch} S {args.seq} aux {args.aux} {args.dtype}", "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "unit": "ms/step"}
    for k, v in times.items():
        res[k] = {"median": round(statistics.median(v), 4), "min": min(v), "max": max(v), "rounds": v, "last_loss": losses[k]}
    res["difference_of_medians"] = round(res["eager_opt"]["median"] - res["graphed_opt"]["median"], 4)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
