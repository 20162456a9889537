"""Fused gradient accumulation, the parts that need no GPU: the gradient sink's state machine driven by a
stand-in encoder (write, then add, then report once; fallback on a foreign ``.grad``; reset by ``step()``; the two-node setting of the
cutoff step undone when its pass ends or its forward raises), GradSync's pass count on two gloo ranks, the rule that picks the path in ``build_optimizer``, and the header / binding agreement
of the new entry points and of ``mtvaf_layer_grads_t::accumulate``."""
import ctypes
import os
import socket
import sys
import types

import pytest
import torch

import abi_header as H

NEW_SYMBOLS = ("mtvaf_gemm_f32p_dw_group_acc", "mtvaf_gemm_f32_dw_group_acc", "mtvaf_gemm_bf16x_dw_group_acc")
PLANNER_QUERY = "mtvaf_gemm_bf16x_dw_group_pieces"


class _Layer(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(n, n))
        self.b = torch.nn.Parameter(torch.zeros(n))

    def ordered_params(self):
        return [self.w, self.b]


class _Store:
    """The flat gradient buffer of one layer and its persistent views (modeling_bert._LayerStore's contract with the sink)."""

    def __init__(self, layer):
        ps = layer.ordered_params()
        self.grad = torch.zeros(sum(p.numel() for p in ps))
        self._gv, off = [], 0
        for p in ps:
            self._gv.append(self.grad[off:off + p.numel()].view(p.shape))
            off += p.numel()

    def grad_views(self):
        return self._gv


class _Encoder(torch.nn.Module):
    """What engine._native_backward does with the sink, on the CPU: acquire with can_accumulate, write or add into the flat views,
    install them as .grad itself, hand autograd None, report every layer newest first."""

    def __init__(self, L=2, n=3):
        super().__init__()
        from mtvaf_amd.models.modeling_bert import GradSink
        self.layer = torch.nn.ModuleList([_Layer(n) for _ in range(L)])
        self._stores = [_Store(l) for l in self.layer]
        self._sink = GradSink(self._stores)
        self.log = []  # (accumulate, fast) of every node that ran

    def forward(self, x):
        enc = self

        class F(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, *params):
                ctx.save_for_backward(x)
                enc._sink.node_created()
                return x.sum() * sum(p.sum() for p in params)

            @staticmethod
            def backward(ctx, g):
                (x,) = ctx.saved_tensors
                params = [p for l in enc.layer for p in l.ordered_params()]
                sink = enc._sink
                views = sink.acquire(params, can_accumulate=True) if sink.accumulate_passes else sink.acquire(params)
                acc = bool(views is not None and sink.accumulate)
                enc.log.append((acc, sink.fast))
                out = [None] * len(params)
                j = len(params)
                for li in range(len(enc.layer) - 1, -1, -1):
                    for p in reversed(enc.layer[li].ordered_params()):
                        j -= 1
                        val = torch.full_like(p, float(x.sum())) * g
                        if views is None:
                            out[j] = val
                        elif acc:
                            views[j].add_(val)
                        else:
                            views[j].copy_(val)
                            p.grad = views[j]
                    sink.layer_done(li)
                return (None, *out)

        return F.apply(x, *[p for l in self.layer for p in l.ordered_params()])


def _params(enc):
    return [p for l in enc.layer for p in l.ordered_params()]


def test_sink_writes_then_accumulates_then_reports_once():
    enc = _Encoder()
    sink = enc._sink
    fired = []
    sink.on_layer_done = lambda li, flat: fired.append((li, None if flat is None else flat.clone()))
    sink.accumulate_passes = 3
    xs = [torch.tensor([1.0, 2.0]), torch.tensor([0.5]), torch.tensor([4.0, 4.0])]
    for i, x in enumerate(xs):
        enc(x).backward()
        assert sink._pass == i + 1 and sink.live_nodes == 0
        if i < 2:
            assert fired == [], "a pass before the last one reports nothing"
    assert enc.log == [(False, True), (True, True), (True, True)]
    assert [li for li, _ in fired] == [1, 0], "every layer once, newest first, on the last pass"
    total = sum(float(x.sum()) for x in xs)
    for (li, flat), st in zip(fired, reversed(enc._stores)):
        assert torch.equal(flat, torch.full_like(flat, total)) and torch.equal(st.grad, flat)
    for p, v in zip(_params(enc), [v for st in enc._stores for v in st.grad_views()]):
        assert p.grad.data_ptr() == v.data_ptr() and torch.equal(p.grad, torch.full_like(p, total))


def test_sink_off_is_the_old_rule():
    """accumulate_passes == 0 (the default): a second backward on existing gradients is the fallback, reported with None."""
    enc = _Encoder()
    sink = enc._sink
    fired = []
    sink.on_layer_done = lambda li, flat: fired.append((li, flat is not None))
    assert sink.accumulate_passes == 0 and sink.nodes_per_pass == 1
    enc(torch.tensor([1.0])).backward()
    enc(torch.tensor([2.0])).backward()
    assert enc.log == [(False, True), (False, False)]
    assert fired == [(1, True), (0, True), (1, False), (0, False)]
    for p in _params(enc):
        assert torch.equal(p.grad, torch.full_like(p, 3.0))  # (autograd added the second pass)


def test_sink_falls_back_on_a_foreign_grad():
    enc = _Encoder()
    sink = enc._sink
    fired = []
    sink.on_layer_done = lambda li, flat: fired.append((li, flat is not None))
    sink.accumulate_passes = 2
    enc(torch.tensor([1.0])).backward()
    ps = _params(enc)
    ps[1].grad = ps[1].grad.clone()  # same values, another storage: not the flat view any more
    enc(torch.tensor([2.0])).backward()
    assert enc.log == [(False, True), (False, False)]
    assert fired == [(1, False), (0, False)], "the fallback reports as it always did: every layer, without a flat buffer"
    for p in ps:
        assert torch.equal(p.grad, torch.full_like(p, 3.0))
    # a view of the right storage at the wrong offset is foreign too
    enc2 = _Encoder()
    enc2._sink.accumulate_passes = 2
    enc2(torch.tensor([1.0])).backward()
    p0, p1 = enc2.layer[0].ordered_params()
    p1.grad = enc2._stores[0].grad[:p1.numel()].view(p1.shape)
    enc2(torch.tensor([2.0])).backward()
    assert enc2.log[-1] == (False, False)


def test_sink_falls_back_without_can_accumulate_and_on_frozen_parameters():
    from mtvaf_amd.models.modeling_bert import GradSink
    enc = _Encoder()
    sink = enc._sink
    sink.accumulate_passes = 2
    enc(torch.tensor([1.0])).backward()
    sink._reset_armed = True  # (acquire is called outside a backward pass here: no end-of-pass callback to queue)
    assert sink.acquire(_params(enc)) is None and sink.fast is False and sink.accumulate is False  # (a caller that cannot add)
    sink._pass_done()
    enc.layer[0].b.requires_grad_(False)
    sink._reset_armed = True
    assert sink.acquire(_params(enc), can_accumulate=True) is None and sink.fast is False
    sink._pass_done()
    assert isinstance(sink, GradSink)


def test_sink_resets_after_step_and_when_gradients_were_cleared():
    enc = _Encoder()
    sink = enc._sink
    fired = []
    sink.on_layer_done = lambda li, flat: fired.append(li)
    sink.accumulate_passes = 2
    for x in (1.0, 2.0):
        enc(torch.tensor([x])).backward()
    assert fired == [1, 0] and sink._pass == 2
    sink.reset_passes()  # (optimizer.step() / zero_grad)
    assert sink._pass == 0 and not sink.last_pass()
    for p in _params(enc):
        p.grad = None
    del fired[:]
    enc(torch.tensor([3.0])).backward()
    assert fired == [] and enc.log[-1] == (False, True)
    enc(torch.tensor([4.0])).backward()
    assert fired == [1, 0] and enc.log[-1] == (True, True)
    assert torch.equal(enc.layer[0].w.grad, torch.full((3, 3), 7.0))
    # gradients set to None by somebody who did not tell the sink: the first node of the next pass starts a new accumulation
    for p in _params(enc):
        p.grad = None
    del fired[:]
    enc(torch.tensor([1.0])).backward()
    assert fired == [] and sink._pass == 1


def test_optimizer_step_and_zero_grad_reset_the_pass_count():
    from mtvaf_amd.optim import AdamW
    enc = _Encoder()
    enc._sink.accumulate_passes = 2
    opt = AdamW.__new__(AdamW)
    opt._encoder = enc
    enc._sink._pass = 2
    opt._new_accumulation()
    assert enc._sink._pass == 0
    with pytest.raises(ValueError):
        AdamW([torch.nn.Parameter(torch.zeros(2))], accumulation_steps=-1)
    with pytest.raises(ValueError, match="needs `model`"):
        AdamW([torch.nn.Parameter(torch.zeros(2))], accumulation_steps=2)


def test_two_node_pass_shares_the_buffers_and_is_undone():
    enc = _Encoder()
    sink = enc._sink
    fired = []
    sink.on_layer_done = lambda li, flat: fired.append((li, flat is not None))
    sink.begin_two_node_pass()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (1, 2)
    (enc(torch.tensor([1.0])) + enc(torch.tensor([2.0]))).backward()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (0, 1), "undone when the pass ended"
    assert enc.log == [(False, True), (True, True)] and fired == [(1, True), (0, True)]
    assert torch.equal(enc.layer[1].w.grad, torch.full((3, 3), 3.0))
    # ended by hand (forward_with_cutoff, when its forward raises): back at once; a second begin does not lose the saved setting
    sink.begin_two_node_pass()
    sink.begin_two_node_pass()
    sink.end_two_node_pass()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (0, 1) and sink._two_node_saved is None
    sink.end_two_node_pass()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (0, 1)
    # accumulation over passes stays on where it was on
    sink.accumulate_passes = 4
    sink.begin_two_node_pass()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (4, 2)
    sink.end_two_node_pass()
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (4, 1)


def test_forward_with_cutoff_restores_the_sink_when_a_pass_raises():
    from mtvaf_amd.models.bert_model import TVNetSAModel
    from mtvaf_amd.models.modeling_bert import GradSink
    sink = GradSink([])

    class Stub:
        args = types.SimpleNamespace(fused_accumulation=True)
        bert = types.SimpleNamespace(encoder=types.SimpleNamespace(grad_sink=sink))

        def _cutoff_passes(self, *a):
            assert (sink.accumulate_passes, sink.nodes_per_pass) == (1, 2)
            raise KeyError("boom")

    with pytest.raises(KeyError):
        TVNetSAModel.forward_with_cutoff(Stub())
    assert (sink.accumulate_passes, sink.nodes_per_pass) == (0, 1)
    Stub.args = types.SimpleNamespace()  # not opted in: the sink is not touched
    Stub._cutoff_passes = lambda self, *a: (sink.accumulate_passes, sink.nodes_per_pass)
    assert TVNetSAModel.forward_with_cutoff(Stub()) == (0, 1)


@pytest.mark.parametrize("accum,fused,overlap_opt,clip,want", [
    (1, False, True, 0.0, (True, 1)), (1, True, True, 0.0, (True, 1)), (1, False, False, 0.0, (False, 1)),
    (2, False, True, 0.0, (False, 1)), (2, True, True, 0.0, (True, 2)), (4, True, False, 0.0, (False, 4)),
    (2, True, True, 1.0, (False, 2)), (1, False, True, 1.0, (False, 1)), (None, True, True, 0.0, (True, 1)),
])
def test_accumulation_plan_matrix(accum, fused, overlap_opt, clip, want):
    from mtvaf_amd.optim import accumulation_plan
    args = types.SimpleNamespace(gradient_accumulation_steps=accum, overlap_optimizer=overlap_opt, max_grad_norm=clip)
    if fused:
        args.fused_accumulation = True
    assert accumulation_plan(args) == want
    args.max_grad_norm, args.track_grad_norm = 0.0, True
    assert accumulation_plan(args) == (False, want[1])


def test_new_entry_points_agree_with_the_header():
    from mtvaf_amd import hip
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    for name in NEW_SYMBOLS:
        res, args = hip._SIGS[name]
        assert (res, list(args)) == H.signature(name), name
        _, _, proto = H.prototype(name)
        assert [a for _, a in proto][-2:] == ["accumulate", "stream"], name
        assert "accumulate" in H.comment_before(name)
    assert PLANNER_QUERY in hip.exported_symbols()
    assert (hip._SIGS[PLANNER_QUERY][0], list(hip._SIGS[PLANNER_QUERY][1])) == H.signature(PLANNER_QUERY)
    # each is its overwriting entry + the flag
    for new, old in (("mtvaf_gemm_f32p_dw_group_acc", "mtvaf_gemm_f32p_dw_group_colsum"),
                     ("mtvaf_gemm_f32_dw_group_acc", "mtvaf_gemm_f32_dw_group_bias"),
                     ("mtvaf_gemm_bf16x_dw_group_acc", "mtvaf_gemm_bf16x_dw_group")):
        a, b = H.prototype(new)[2], H.prototype(old)[2]
        assert a[:-2] == b[:-1] and a[-1] == b[-1] and a[-2] == ("int", "accumulate")


def test_layer_grads_struct_ends_with_accumulate():
    from mtvaf_amd import hip
    fields = H.structs()["mtvaf_layer_grads_t"]
    assert fields[-1] == ("accumulate", "int")
    assert [n for n, _ in hip.LayerGradsStruct._fields_] == [n for n, _ in fields]
    assert hip.LayerGradsStruct._fields_[-1] == ("accumulate", ctypes.c_int)
    assert hip.LayerGradsStruct().accumulate == 0, "a zero-initialised struct is the overwriting executor"
    assert hip.lib().mtvaf_layer_struct_bytes(1) == ctypes.sizeof(hip.LayerGradsStruct)


# ---- GradSync with a pass count: two gloo ranks, k = 2 ------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = _Encoder(L=3, n=4)
        self.encoder.grad_sink = self.encoder._sink
        self.head = torch.nn.Linear(4, 1)
        self.table = torch.nn.Parameter(torch.ones(64, 8))  # a "large" parameter: exchanged by its own hook

    def forward(self, x):
        return self.encoder(x) + self.head(x[:4]).sum() + (self.table * x).sum()


def _x(rank, i):
    return torch.arange(8, dtype=torch.float32) * (rank + 1) + i


def _sync_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mtvaf_amd.optim import AdamW
    from mtvaf_amd.parallel import GradSync
    torch.manual_seed(0)
    m = _Model()
    sync = GradSync(m, big_numel=256, compress=None)
    opt = AdamW(m.parameters(), lr=1e-3, model=m, grad_sync=sync, accumulation_steps=2)
    sink = m.encoder._sink
    res = {"k": (sync.accumulation_steps, sink.accumulate_passes, opt.accumulation_steps)}
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **kw: (calls.append(int(t.numel())), real(t, *a, **kw))[1]
    flat_numel = m.encoder._stores[0].grad.numel()
    m(_x(rank, 0)).backward()
    res["pass1_collectives"] = list(calls)
    res["pass1"] = [p.grad.tolist() for p in m.parameters()]
    m(_x(rank, 1)).backward()
    res["pass2_layer_collectives"] = sum(1 for n in calls if n == flat_numel)
    res["pass2"] = [p.grad.tolist() for p in m.parameters()]
    res["flat"] = all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(_params(m.encoder), [v for st in m.encoder._stores for v in st.grad_views()]))
    dist.all_reduce = real
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_gradsync_exchanges_nothing_before_the_last_pass():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # single-process oracle: per rank the sum over its two micro-batches; then the mean over ranks
    torch.manual_seed(0)
    ref = _Model()
    local = []
    for r in range(world):
        ref.zero_grad(set_to_none=True)
        ref.encoder._sink.reset_passes()
        firsts = None
        for i in range(2):
            ref(_x(r, i)).backward()
            if i == 0:
                firsts = [p.grad.clone() for p in ref.parameters()]
        local.append((firsts, [p.grad.clone() for p in ref.parameters()]))
    mean = [sum(g) / world for g in zip(*[l[1] for l in local])]
    for r in range(world):
        assert out[r]["k"] == (2, 2, 2), "AdamW.attach hands its pass count to the sink and to GradSync"
        assert out[r]["pass1_collectives"] == [], "nothing is exchanged before the last pass"
        for got, want in zip(out[r]["pass1"], local[r][0]):
            torch.testing.assert_close(torch.tensor(got), want)  # (still this rank's own partial sum)
        assert out[r]["pass2_layer_collectives"] == 3, "one flat buffer per layer on the last pass"
        assert out[r]["flat"]
        for got, want in zip(out[r]["pass2"], mean):
            torch.testing.assert_close(torch.tensor(got), want)
