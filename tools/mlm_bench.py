"""Masked-LM head and masking on one MI355X, the process's default arithmetic.

    python tools/mlm_bench.py [--repeats 5] [--iters 20] [--out profiles/mlm_bench.json]

head:  gather-free decoder + cross entropy forward + backward on cap = default capacity of 32 x 128 at 15 % rows, H 768, V 30522:
       engine.VocabCEFunction at several chunk widths against the eager chain F.linear + F.cross_entropy with autograd on the same
       rows.  Per variant: ms per forward + backward (min .. max over the repeats of an `iters`-long timed loop) and the peak of
       extra device memory during one forward + backward (torch.cuda.max_memory_allocated above the level before the call).
mask:  one mlm.mask_tokens call at 32 x 128 against the collator rule in torch on CPU tensors plus the copies to the device."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtvaf_amd import engine, hip, mlm  # noqa: E402

DEV = "cuda"


def timed(fn, iters, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"ms_min": round(min(out), 4), "ms_max": round(max(out), 4)}


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def head(args):
    B, S, H, V = 32, 128, 768, 30522
    cap = mlm.default_capacity(B * S, 0.15)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(cap, H, generator=g)).to(DEV).requires_grad_(True)
    W = (torch.randn(V, H, generator=g) * 0.02).to(DEV).requires_grad_(True)
    b = torch.zeros(V, device=DEV, requires_grad=True)
    count = int(0.15 * B * S)
    labels = torch.randint(0, V, (cap,), generator=g)
    labels[count:] = -100
    labels = labels.to(DEV)
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)

    def chunked(chunk):
        def run():
            x.grad = W.grad = b.grad = None
            engine.VocabCEFunction.apply(x, W, b, labels, cnt, "mean", chunk)[0].backward()
        return run

    def eager():
        x.grad = W.grad = b.grad = None
        F.cross_entropy(F.linear(x, W, b), labels, ignore_index=-100).backward()

    res = {"rows": cap, "live_rows": count, "H": H, "V": V, "variants": {}}
    for name, fn in [("eager", eager)] + [(f"chunk_{c}", chunked(c)) for c in args.chunks + [V]]:
        r = timed(fn, args.iters, args.repeats)
        r["peak_extra_bytes"] = peak_extra(fn)
        res["variants"][name] = r
        print(name, r, flush=True)
    lc = float(engine.VocabCEFunction.apply(x, W, b, labels, cnt, "mean", engine.VOCAB_CE_CHUNK)[0].detach())
    le = float(F.cross_entropy(F.linear(x, W, b), labels, ignore_index=-100).detach())
    res["loss_chunked"], res["loss_eager"], res["default_chunk"] = lc, le, engine.VOCAB_CE_CHUNK
    res["workspace_bytes_default"] = hip.vocab_ce_workspace_bytes(cap, H, V, engine.VOCAB_CE_CHUNK)
    return res


def host_collator(ids, att, special, p, mask_id, V):
    """DataCollatorForLanguageModeling.torch_mask_tokens restated on CPU tensors"""
    labels = ids.clone()
    prob = torch.full(ids.shape, p)
    prob.masked_fill_(special | (att == 0), 0.0)
    sel = torch.bernoulli(prob).bool()
    labels[~sel] = -100
    rep = torch.bernoulli(torch.full(ids.shape, 0.8)).bool() & sel
    out = ids.clone()
    out[rep] = mask_id
    rnd = torch.bernoulli(torch.full(ids.shape, 0.5)).bool() & sel & ~rep
    out[rnd] = torch.randint(V, ids.shape)[rnd]
    return out, labels


def masking(args):
    B, S, V = 32, 128, 30522
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, V, (B, S), generator=g)
    lengths = torch.randint(20, S + 1, (B,), generator=g)
    att = (torch.arange(S)[None, :] < lengths[:, None]).long()
    ids[:, 0] = 101
    ids[att == 0] = 0
    special = (ids == 101) | (ids == 0)
    ids_d, att_d = ids.to(DEV), att.to(DEV)

    def device():
        mlm.mask_tokens(ids_d, att_d, mask_token_id=103, vocab_size=V, special_ids=(0, 101, 102, 103))

    def wall(fn):
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / args.iters)
        return {"ms_min": round(min(out), 4), "ms_max": round(max(out), 4)}

    def host():
        out, labels = host_collator(ids, att, special, 0.15, 103, V)
        return out.to(DEV), labels.to(DEV)

    device(), host()
    return {"B": B, "S": S, "device_mask_tokens_wall": wall(device), "device_mask_tokens_gpu": timed(device, args.iters, args.repeats),
            "host_collator_plus_copy_wall": wall(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--chunks", type=int, nargs="*", default=[1024, 4096, 8192])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "compute": hip.COMPUTE, "head": head(args), "mask": masking(args)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
