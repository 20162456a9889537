"""What `mtvaf_amd.optim.AdamW` launches, recorded: the one recorder of the optimizer tests, and the fixed scenarios whose traces
`tests/golden/adamw_launch_trace.json` pins (test_optim_trace_gpu.py compares, tools/adamw_trace.py --write regenerates).

A trace holds, per call of a `mtvaf_amd.hip` wrapper the optimizer uses (and of the `mtvaf_amd.engine` calls that hand out and stamp
the weight images): the name, dtype and length of every tensor, the lengths of every list of tensors, every Python scalar exactly
(`float.hex()`), the numeric columns of segment tables and `mats`, which optional arguments were given, and whether the call went to
`hip.STREAM_OVERRIDE`.  No pointer, nothing that differs between two runs of one tree."""
import contextlib
import json
import os

import torch

HIP_PREFIXES = ("adamw", "sam_", "grad_sqnorm", "grad_clip", "swap_f32")
ENGINE_CALLS = ("planes_written", "shadow_written", "planes_rewrite", "planes_for_update", "shadow_for_update", "invalidate_weight_images")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_launch_trace.json")


def optimizer_wrappers(hip_mod):
    """Every wrapper of mtvaf_amd.hip that launches for the optimizer."""
    return [k for k in dir(hip_mod) if k.startswith(HIP_PREFIXES) and callable(getattr(hip_mod, k)) and k != "grad_sqnorm_slots"]


@contextlib.contextmanager
def recorded(hip_mod=None, names=None, record=lambda name, a, k: name, engine_calls=()):
    """`names` of mtvaf_amd.hip (default: every wrapper that launches for the optimizer) and `engine_calls` of mtvaf_amd.engine,
    replaced for the block by wrappers that append `record(name, args, kwargs)` to the list this yields and then call through."""
    from mtvaf_amd import engine
    if hip_mod is None:
        from mtvaf_amd import hip as hip_mod
    targets = [(hip_mod, k) for k in (optimizer_wrappers(hip_mod) if names is None else names)] + [(engine, k) for k in engine_calls]
    real = [(mod, k, getattr(mod, k)) for mod, k in targets]
    calls = []

    def wrap(name, fn):
        def f(*a, **k):
            calls.append(record(name, a, k))
            return fn(*a, **k)
        return f
    try:
        for mod, k, fn in real:
            setattr(mod, k, wrap(k, fn))
        yield calls
    finally:
        for mod, k, fn in real:
            setattr(mod, k, fn)


def recorded_updates():
    """The update wrappers, recorded as (wrapper, with average, with shadow, with clip state, `ema` passed at all)."""
    return recorded(names=("adamw", "adamw_planes", "adamw_multi", "swap_f32"),
                    record=lambda name, a, k: (name, k.get("ema") is not None, k.get("p_bf16") is not None, k.get("clip") is not None,
                                               "ema" in k))


# ---- the launch trace ----------------------------------------------------------------------------------------------------
def _enc(x):
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return x.hex()
    if torch.is_tensor(x):
        return [str(x.dtype).replace("torch.", ""), x.numel()]
    if isinstance(x, (list, tuple)):
        if x and all(torch.is_tensor(t) for t in x):
            return {"numels": [t.numel() for t in x]}
        return [_enc(t) for t in x]
    return type(x).__name__  # (engine.LayerWeights)


def _trace_record(hip_mod):
    return lambda name, a, k: [name, [_enc(x) for x in a], {key: _enc(k[key]) for key in sorted(k)}, hip_mod.STREAM_OVERRIDE is not None]


def traced(hip_mod=None):
    if hip_mod is None:
        from mtvaf_amd import hip as hip_mod
    return recorded(hip_mod, record=_trace_record(hip_mod), engine_calls=ENGINE_CALLS)


MODES = ("planes", "flat", "bf16")


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def scenarios():
    """-> {scenario: function that runs it and returns its calls}, in the order of the golden file: every scenario on
    test_ema_gpu's 2-layer model and batch, two optimizer steps each (the second with state, counters at 1 and a non-zero EMA
    decay)."""
    from mtvaf_amd import hip
    from mtvaf_amd.optim import DEFAULT_NO_DECAY, AdamW, finetune_param_groups, schedule_table
    from test_ema_gpu import _batch, _mode, _model
    from test_sam_gpu import _on_the_image_path
    reg = {}

    def plain_steps(m, opt, batch, steps=2, passes=1):
        for _ in range(steps):
            for _ in range(passes):
                m(**batch).loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)

    def sam_steps(m, opt, batch, steps=2):
        for _ in range(steps):
            m(**batch).loss.backward()
            opt.perturb()
            m(**batch).loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)

    def scenario(name, mode, drive=plain_steps, groups=None, plans=True, on_images=True, before=None, **kw):
        def run():
            with _mode(mode), (before() if before else contextlib.nullcontext()) as extra:
                m, cfg = _model()
                batch = _batch(cfg)
                if extra is not None:
                    kw["grad_sync"] = extra(m)
                opt = AdamW(m.parameters() if groups is None else groups(m), lr=1e-3, model=m, **kw)
                if not plans:
                    opt.SEGMENT_PLANS = False
                    opt._map_layers()
                with traced(hip) as calls:
                    drive(m, opt, batch)
                torch.cuda.synchronize()
                if mode == "planes" and on_images:  # the images were in use: the planes forms are in the trace
                    assert _on_the_image_path(m, mode), name
                assert calls, name
                return list(calls)
        assert f"{name}[{mode}]" not in reg
        reg[f"{name}[{mode}]"] = run

    split = lambda m: finetune_param_groups(m, 1e-3, no_decay=DEFAULT_NO_DECAY)
    table = lambda **kw: schedule_table(lambda t: 1.0 / (1.0 + t), 8, **kw)
    for mode in MODES:
        scenario("plain", mode)
        scenario("overlap", mode, overlap=True)
        scenario("clip", mode, max_grad_norm=1.0)
        scenario("ema", mode, ema_decay=0.9)
        scenario("groups", mode, groups=split)
        scenario("groups_tensor_by_tensor", mode, groups=split, plans=False)
        scenario("device_schedule_clip_ema", mode, max_grad_norm=1.0, ema_decay=0.9, device_schedule=table(ema_decay=0.9))
        scenario("device_schedule_groups", mode, groups=split, device_schedule=table())
        scenario("sam_clip", mode, drive=sam_steps, sam_rho=0.05, max_grad_norm=1.0)
        scenario("sam", mode, drive=sam_steps, sam_rho=0.05)

    scenario("accumulation_overlap", "planes", drive=lambda m, o, b: plain_steps(m, o, b, passes=2), accumulation_steps=2, overlap=True)

    for name, kw in (("load_state_dict", {}), ("load_state_dict_ema", dict(ema_decay=0.9))):
        def reloaded(m, opt, batch, kw=kw):
            import copy
            plain_steps(m, opt, batch, steps=1)
            fresh = AdamW(m.parameters(), lr=1e-3, model=m, **kw)
            fresh.load_state_dict(copy.deepcopy(opt.state_dict()))
            plain_steps(m, fresh, batch, steps=1)
        scenario(name, "planes", drive=reloaded, **kw)

    def swapped(m, opt, batch):
        plain_steps(m, opt, batch, steps=1)
        opt.swap_ema()
        opt.swap_ema()
        plain_steps(m, opt, batch, steps=1)
    scenario("swap_ema", "planes", drive=swapped, ema_decay=0.9)

    def unperturbed(m, opt, batch):
        m(**batch).loss.backward()
        opt.perturb()
        opt.unperturb()
        opt.zero_grad(set_to_none=True)
        sam_steps(m, opt, batch, steps=1)
    scenario("unperturb", "planes", drive=unperturbed, sam_rho=0.05)

    def graphed(m, opt, batch):  # (the recorder is installed before the capture: the replays launch nothing through Python)
        from mtvaf_amd.graph import GraphedTrainStep
        g = GraphedTrainStep(m, batch, optimizer=opt)
        try:
            for _ in range(2):
                g(**batch)
                opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            assert opt.schedule_count == 2
        finally:
            g.close()
    scenario("graphed_step", "planes", drive=graphed, on_images=False, max_grad_norm=1.0, ema_decay=0.9,
             device_schedule=table(ema_decay=0.9))

    @contextlib.contextmanager
    def one_rank_group():
        """A forced one-rank GradSync: the updates hang off the communication stream's per-layer hook."""
        import torch.distributed as dist
        from mtvaf_amd.parallel import GradSync
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        try:
            yield lambda m: GradSync(m, force=True, seed_per_rank=False)
        finally:
            dist.destroy_process_group()
    scenario("overlap_gradsync", "planes", on_images=False, before=one_rank_group, overlap=True)
    return reg


def run_scenarios():
    return {key: run() for key, run in scenarios().items()}


def dumps(traces) -> str:
    """One call per line, scenarios in the order they ran."""
    body = []
    for key, calls in traces.items():
        lines = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in calls)
        body.append(f" {json.dumps(key)}: [\n{lines}\n ]")
    return "{\n" + ",\n".join(body) + "\n}\n"
