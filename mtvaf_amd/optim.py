"""Optimizer / LR schedule of the reference trainers, for the drop-in models.

``AdamW`` below is the hand-written optimizer of the path: torch.optim.AdamW semantics on the HIP kernels of
``csrc/optim.hip`` -- ONE launch per encoder layer over the layer's flat parameter / gradient / moment buffers, one
multi-tensor launch per 48 remaining tensors -- and, with ``overlap=True``, the per-layer updates are enqueued from
inside the backward pass (behind the layer's gradient all-reduce on the communication stream under ``GradSync``, behind
its weight-gradient kernels on the second stream otherwise), so the HBM-bound update runs next to the MFMA-bound rest of
the backward pass instead of after it.

``modules/train.py::SATrainer2.multiModal_before_train`` (:894-926) builds three AdamW parameter groups by
NAME (encoder ``bert*`` at ``args.lr``; ``encoder_conv*`` / ``gates*`` at ``args.lr``; ``crf*`` / ``fc*`` at
5e-2; weight decay 1e-2 everywhere), freezes ``image_model*`` and attaches a linear warm-up / linear decay
schedule; ``bert_before_train`` (:887-892) is the text-only variant (one group, all parameters).  The same
grouping is reproduced here (``reference_param_groups`` / ``build_optimizer``) on top of ``AdamW`` below, so a step of
the reference trainer costs what ``bench.py`` measures.

``finetune_param_groups`` is the usual BERT fine-tuning recipe on the same partition (no weight decay on biases and LayerNorm
weights, lr decaying with depth; ``args.no_decay`` / ``args.layer_lr_decay``): an encoder layer then holds two parameter groups
and is still ONE launch -- the segmented kernels of ``csrc/optim.hip`` take lr and weight decay per stretch of the layer's buffer
(``layer_segments``).

Reference quirk kept on purpose: ``projectors.*``, ``img_classifier.*`` and ``aux_img_classifier.*`` match no
group (the second group looks for the long-gone ``gates``), so the reference never updates them.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional

import torch

from . import hip


def ema_decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """Decay of EMA update number ``t`` (0-based: the count of EMA updates already applied to that tensor or layer).

    ``t == 0`` -> 0: on the zero-initialised average ``fmaf(1, p - 0, 0)`` is ``p`` exactly, so the average starts as the
    parameters after their first update, written by the update kernel on the update's own stream -- no copy.  Then, with
    ``warmup``, ``min(decay, (1 + t) / (10 + t))`` (the early average follows the weights instead of remembering the
    initialisation for 1 / (1 - decay) steps); without, ``decay``."""
    if t <= 0:
        return 0.0
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class ScheduleTable:
    """What ``schedule_table`` returns: the per-step hyper-parameters of a whole run, as the bytes the device reads.

    ``rows`` is a numpy record array, one 24-byte row per optimizer step 1 .. T (``lr_factor`` float64; ``bc1``, ``bc2_sqrt``,
    ``ema_omd`` float32; ``pad``) -- row ``t - 1`` is update ``t``.  ``lr_factors`` are the T + 1 values ``factor(0) .. factor(T)`` on the
    host (``factor(t)`` is what ``group["lr"]`` shows after update ``t``); ``num_steps`` is the T that was asked for."""
    FIELDS = [("lr_factor", "<f8"), ("bc1", "<f4"), ("bc2_sqrt", "<f4"), ("ema_omd", "<f4"), ("pad", "<i4")]

    def __init__(self, rows, lr_factors, num_steps, betas, ema_decay, ema_warmup):
        self.rows, self.lr_factors, self.num_steps = rows, lr_factors, int(num_steps)
        self.betas, self.ema_decay, self.ema_warmup = (float(betas[0]), float(betas[1])), float(ema_decay), bool(ema_warmup)

    def __len__(self):
        return len(self.rows)


def schedule_table(factor, num_steps: int, betas=(0.9, 0.999), ema_decay: float = 0.0, ema_warmup: bool = True) -> ScheduleTable:
    """The table behind ``AdamW(device_schedule=...)``: everything of optimizer steps 1 .. ``num_steps`` that changes from step to
    step, computed here with the host's own expressions so that the device reads the host's bits.

    ``factor`` is the function a ``LambdaLR`` would be given.  In the loop ``opt.step(); sched.step()`` update ``t`` runs at
    ``base_lr * factor(t - 1)`` (the scheduler's constructor applies ``factor(0)``, its ``t``-th ``step()`` applies ``factor(t)`` for
    the NEXT update), so row ``t`` holds ``factor(t - 1)``; ``bc1 = 1 - beta1 ** t`` and ``bc2_sqrt = (1 - beta2 ** t) ** 0.5`` rounded
    to float once, as ``mtvaf_amd.hip`` hands them to the kernels; ``ema_omd = 1 - ema_decay_at(t - 1, ema_decay, ema_warmup)``
    likewise (``AdamW._ema_omd``)."""
    import numpy as np
    T = int(num_steps)
    if T < 1:
        raise ValueError("schedule_table: num_steps must be >= 1")
    b1, b2 = betas
    lr_factors = [float(factor(t)) for t in range(T + 1)]
    rows = np.zeros(T, dtype=ScheduleTable.FIELDS)
    for t in range(1, T + 1):
        rows[t - 1] = (lr_factors[t - 1], float(1.0 - b1 ** t), float((1.0 - b2 ** t) ** 0.5),
                       float(1.0 - ema_decay_at(t - 1, ema_decay, ema_warmup)), 0)
    return ScheduleTable(rows, lr_factors, T, betas, ema_decay, ema_warmup)


class ScheduleMirror:
    """The scheduler ``build_optimizer`` returns beside an ``AdamW(device_schedule=...)``: the kernels take their learning rate from
    the device's table, so ``step()`` launches and computes nothing -- it advances a host count and shows readers of
    ``group["lr"]`` the table's value for the next update (``base_lr * factor(count)``, what a ``LambdaLR`` would have written)."""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.last_epoch = optimizer.schedule_count
        self._show()

    def _show(self):
        f = self.optimizer.device_schedule.lr_factors
        for g in self.optimizer.param_groups:
            g["lr"] = g["initial_lr"] * f[min(self.last_epoch, len(f) - 1)]

    def step(self):
        self.last_epoch += 1
        self._show()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, state):
        self.last_epoch = int(state["last_epoch"])
        self._show()


MAX_SEGMENTS = 16  # of one segmented launch (csrc/optim.hip, ADAM_MAXSEG): an encoder layer has 16 parameters


def _same_lr_wd(a, b) -> bool:
    return a is b or (a["lr"], a["weight_decay"]) == (b["lr"], b["weight_decay"])


def layer_segments(offsets, numels, hypers, same=_same_lr_wd):
    """The plan of ONE launch over a flat buffer whose tensors do not share their hyper-parameters (``hip.adamw_seg``).

    Tensor i lies at elements ``[offsets[i], offsets[i] + numels[i])`` and is trained with the mapping ``hypers[i]`` (keys ``lr``,
    ``weight_decay``, ``betas``, ``eps``: a parameter group, or a plain dict).  -> ``[(end element, hypers of the segment), ...]`` in
    buffer order, adjacent tensors merged where ``same(a, b)`` (default: equal ``(lr, weight_decay)``); or None where one launch
    cannot do it: the tensors do not tile the buffer from 0 without gaps, ``betas`` or ``eps`` differ (they belong to the launch), an
    end other than the last is not a multiple of 4 elements (the kernel works in float4s), or more than 16 segments remain.
    Pure host logic.  The optimizer passes ``same = identity of the group``: two groups whose lr are equal today need not stay so
    under a scheduler, and ``group["lr"]`` is read at every update."""
    order = sorted(range(len(offsets)), key=lambda i: offsets[i])
    if not order:
        return None
    h0 = hypers[order[0]]
    segs, end = [], 0
    for i in order:
        h = hypers[i]
        if offsets[i] != end or numels[i] <= 0 or tuple(h["betas"]) != tuple(h0["betas"]) or h["eps"] != h0["eps"]:
            return None
        end += numels[i]
        if segs and same(segs[-1][1], h):
            segs[-1] = (end, segs[-1][1])
        else:
            segs.append((end, h))
    if len(segs) > MAX_SEGMENTS or any(e % 4 for e, _ in segs[:-1]):
        return None
    return segs


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, bias correction, no amsgrad) on the gfx950 kernels.

    ``attach(model)`` (or ``model=`` at construction) lets the optimizer see the encoder's per-layer flat buffers
    (``BertEncoder._stores``): a layer whose 16 parameters sit in one parameter group is updated by ONE launch -- and so is a layer
    whose parameters sit in several groups that differ in ``lr`` and ``weight_decay`` only (biases and LayerNorm weights without
    weight decay, ``finetune_param_groups``): the layer's buffer is then updated as up to 16 segments (``layer_segments``,
    ``hip.adamw_seg`` / ``hip.adamw_planes_seg``) on every path the single-group launch takes -- ``step()``, ``overlap=True``, under
    ``GradSync``, with clipping, the averaged weights, the bf16 shadow and the plane images.  Groups of one layer that differ in
    ``betas`` or ``eps`` leave that layer to the tensor-by-tensor launches.

    ``overlap=True``: layers are updated from inside ``loss.backward()`` as soon as their gradients are final (after
    the all-reduce under data parallelism).  Contract: every backward pass is followed by exactly one ``step()`` before
    the next backward (the reference trainer's flow with gradient_accumulation_steps = 1, modules/train.py:620-625);
    a second backward without a ``step()`` raises -- with or without ``zero_grad`` in between, so gradient accumulation
    (gradient_accumulation_steps > 1, train.py:616-625) cannot silently train the encoder on one micro-batch: use
    ``overlap=False`` for it (``build_optimizer`` does), or ``accumulation_steps=k`` (fused accumulation, DESIGN.md 4.21: the first k - 1
    backward passes add into the flat gradient buffers and update nothing, pass k updates each layer from inside its backward, a
    (k + 1)-th pass without ``step()`` raises; with ``overlap=False`` the k passes simply share the flat buffers).  ``step()`` then only updates what is left (embeddings, heads,
    prompt generator) and layers that could not take the fast path.

    ``max_grad_norm > 0``: gradients are clipped by their global L2 norm (``torch.nn.utils.clip_grad_norm_``'s rule) INSIDE the
    update kernels: ``step()`` launches one multi-tensor sum of squares (double) over every gradient it is about to apply and a
    one-block finalize that leaves ``{norm, coefficient, finite}`` on the device, then every update through the ``*_dev`` entry
    points, which scale the gradient by that coefficient -- no host synchronisation, no pass that rewrites the gradients
    (``.grad`` keeps its unclipped values).  ``track_grad_norm=True`` alone reports the norm without clipping.  Either switch
    makes ``last_grad_norm`` (0-dim device tensor, the pre-clip norm) and ``skipped_steps`` (device int32) live; with
    ``skip_nonfinite`` (default) a step whose norm is inf / NaN writes NOTHING -- parameters, moments, bf16 shadows and plane
    images keep their bits -- and is counted in ``skipped_steps``.  The host cannot know that without a sync, so the step
    counters still advance: after a skipped step the bias correction is one step ahead.
    ``skip_nonfinite=False`` keeps torch's behaviour (the NaN coefficient reaches the parameters).  With both switches off
    ``step()`` issues exactly the launches it always did, and ``skip_nonfinite`` has nothing to act on.  A global norm is not
    known while layers are still being updated inside backward: together with ``overlap=True`` either switch raises.

    ``ema_decay > 0``: every update kernel also keeps an exponential moving average of the parameter it has just written,
    ``ema += (1 - d) * (p_new - ema)`` with ``d = ema_decay_at(t, ema_decay, ema_warmup)`` -- on every path: the per-layer flat update
    and its plane-image form, the tensor-by-tensor launches, with and without clipping, and ``overlap=True`` from inside backward.
    ``state[p]["ema"]`` is the average (an encoder layer's are views of one flat buffer, like ``exp_avg``) and ``state[p]["ema_step"]``
    the number of updates it has seen, so both travel through ``state_dict()`` / ``load_state_dict()``; a checkpoint written without
    them starts the average at the next step.  ``ema_decay`` is a setting of the optimizer like ``max_grad_norm``, not of a
    parameter group: it is not in ``defaults`` and a group cannot override it.  ``swap_ema()`` exchanges the parameters with their
    averages (and back: bit for bit), ``averaged_parameters()`` does so around a block, ``ema_state_dict(model)`` is the averaged
    model to save.  While the averages are swapped in (``ema_swapped``) ``step()`` and the backward hook raise.  On a step the
    non-finite skip drops, the average keeps its bits but ``ema_step`` advances like the step counters (same caveat).  At
    ``ema_decay == 0`` (default) nothing is allocated and ``step()`` issues the launches it always did.

    ``device_schedule=schedule_table(...)``: the step's own hyper-parameters -- the lr factor, both bias corrections and the
    average's ``1 - decay`` -- live on the device.  ``step()`` first launches ``hip.adamw_sched_advance`` (a device
    step counter += 1, that step's table row -> a fixed 32-byte block) and then the ``*_sched`` form of every update it would have
    launched, which take the group's BASE lr (``group["initial_lr"]``, as a double) and read the rest from that block: no kernel
    argument changes from step to step, so ``mtvaf_amd.graph.GraphedTrainStep(model, batch, optimizer=opt)`` captures the whole
    step.  Same bits as ``AdamW`` + ``LambdaLR(factor)``.  The host keeps a mirror of the counter (``schedule_count``, one increment
    per ``step()`` or replay -- ``host_step()`` is that bookkeeping alone and launches nothing) and raises BEFORE a step past the
    table's end; on the device such a step would write nothing.  Limits, checked at construction or at the first step: one
    ``betas`` for all groups (the bias corrections are the table's), every parameter on one step count (and one EMA update count),
    ``overlap=False``, and the table's ``ema_decay`` / ``ema_warmup`` are the optimizer's.  ``group["lr"]`` is not read by the
    kernels any more; a scheduler may still write it for readers (``ScheduleMirror``, or a ``LambdaLR`` with the table's factor)
    and ``assert_schedule_agrees()`` compares the two on demand.

    ``sam_rho > 0``: sharpness-aware minimisation (Foret et al. 2021).  The loop is: backward, ``perturb()``, forward
    and backward again, ``step()`` -- ``mtvaf_amd.sam.SharpnessAware`` runs it.  ``perturb()`` moves every parameter the step would
    update to ``p + sam_rho * g / (|g| + 1e-12)`` (global norm in double on the device, no host synchronisation), keeps the weights
    aside (4 B per parameter, allocated at the first call) and discards the first pass's gradients; an encoder layer is ONE launch
    that also rewrites the bf16 shadow or the plane images, so the second pass's GEMMs read the perturbed weights.  ``step()``
    restores the weights bit for bit and then is the step it always was (clipping, averages, segments); where clipping can drop
    the step on the device the restore rewrites the images too.  ``last_sam_norm`` (0-dim device view) and ``sam_skipped`` (device
    int32: a non-finite norm leaves the weights alone) report.  ``step()`` without ``perturb()`` is a plain step; ``unperturb()``
    restores without one.  Like ``max_grad_norm`` a setting of the optimizer, not in ``defaults``; nothing of it is in
    ``state_dict()``.  Raises: ``overlap=True``, ``accumulation_steps > 1``, ``device_schedule`` / a ``GraphedTrainStep``, a
    ``GradSync`` with several ranks, ``perturb()`` while the averages are swapped in or twice without ``step()``,
    ``load_state_dict`` while perturbed.  At ``sam_rho == 0`` (default) nothing is allocated and ``step()`` issues the launches it
    always did.

    Checkpoints: ``state_dict()`` / ``load_state_dict()`` are torch.optim's; the flat per-layer moment buffers are
    rebuilt from the loaded per-parameter ``exp_avg`` / ``exp_avg_sq`` / ``step`` entries on the first update.  Under a device
    schedule loading also sets the host mirror and the device counter to the loaded step count."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 model: Optional[torch.nn.Module] = None, overlap: bool = False, grad_sync=None, max_grad_norm: float = 0.0,
                 track_grad_norm: bool = False, skip_nonfinite: bool = True, ema_decay: float = 0.0, ema_warmup: bool = True,
                 accumulation_steps: int = 1, device_schedule: Optional[ScheduleTable] = None, sam_rho: float = 0.0):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0) or weight_decay < 0.0:
            raise ValueError("invalid AdamW hyper-parameters")
        sam_rho = float(sam_rho or 0.0)
        if not (0.0 <= sam_rho < float("inf")):  # (NaN fails both comparisons)
            raise ValueError("sam_rho must be finite and >= 0 (0: no sharpness-aware step)")
        if sam_rho > 0.0:
            who = "mtvaf_amd.optim.AdamW(sam_rho > 0)"
            if overlap:
                raise ValueError(f"{who} needs overlap=False: layers updated from inside the first backward pass would move the "
                                 "weights before perturb() has read them (build_optimizer arranges it)")
            if int(accumulation_steps or 1) > 1:
                raise ValueError(f"{who} with accumulation_steps > 1 is not supported: perturb() discards the first pass's gradients, "
                                 "fused accumulation would add them to the second pass's; use accumulation_steps=1")
            if device_schedule is not None:
                raise ValueError(f"{who} with device_schedule is not supported: a SAM step is two eager passes with perturb() between "
                                 "them and cannot be captured; use a LambdaLR (linear_schedule_with_warmup) on the host")
        self.sam_rho = sam_rho
        self.sam_perturbed = False  # True between perturb() and the step() that restores the weights
        self.last_sam_norm = None   # 0-dim view of _sam_state[0]: the gradient norm the last perturb() scaled by
        self.sam_skipped = None     # device int32: perturb() calls whose norm was not finite (the weights were left alone)
        self._sam_state = None      # device {norm, scale, finite, 0}: written by hip.sam_finalize, read by the perturb kernels
        self._sam_partials = None
        self._sam_backup = {}       # ("layer", li) / id(parameter) -> the weights before perturb(): 4 B per parameter, kept
        self._sam_record = None     # what the last perturb() wrote: ([(store, backup)], [parameters], [backups])
        max_grad_norm = float(max_grad_norm or 0.0)
        if max_grad_norm != max_grad_norm or max_grad_norm < 0.0:
            raise ValueError("max_grad_norm must be >= 0 (0: no clipping)")
        if overlap and (max_grad_norm > 0.0 or track_grad_norm):
            raise ValueError("mtvaf_amd.optim.AdamW: max_grad_norm / track_grad_norm need overlap=False -- the global gradient norm "
                             "is not known while layers are still being updated from inside the backward pass")
        ema_decay = float(ema_decay or 0.0)
        if not (0.0 <= ema_decay < 1.0):  # (NaN fails both comparisons)
            raise ValueError("ema_decay must be in [0, 1) (0: no averaged weights)")
        self.ema_decay = ema_decay
        self.ema_warmup = bool(ema_warmup)
        self.ema_swapped = False  # True: the parameters hold the averages, state[p]["ema"] the training weights (swap_ema)
        self.max_grad_norm = max_grad_norm
        self.track_grad_norm = bool(track_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_state = None     # device {norm, coef, finite, 0}: written by the finalize kernel, read by the *_dev updates
        self._clip_partials = None  # device doubles, one per 65536-element chunk of the gradients
        self.last_grad_norm = None  # 0-dim view of _clip_state[0]: the pre-clip global norm of the last step()
        self.skipped_steps = None   # device int32: steps whose norm was not finite (skip_nonfinite)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.overlap = overlap
        accumulation_steps = int(accumulation_steps or 1)
        if accumulation_steps < 1:
            raise ValueError("accumulation_steps must be >= 1")
        if accumulation_steps > 1 and model is None:
            raise ValueError("mtvaf_amd.optim.AdamW: accumulation_steps > 1 is the encoder's fused accumulation and needs `model`")
        self.accumulation_steps = accumulation_steps
        self._encoder = None
        self._layer_group: Dict[int, Optional[dict]] = {}
        self._early = set()
        self._param_layer: Dict[int, int] = {}  # id(parameter) -> encoder layer whose flat state its entries are views of
        self._flat_state: Dict[tuple, dict] = {}  # ("layer", li) -> the layer's flat moment buffers and counters (_layer_state)
        self._background_ok = True
        self.suspended = False    # True: the backward hook does nothing (backward passes that are not followed by step())
        self.device_schedule = None  # a ScheduleTable: the *_sched kernels, hyper-parameters of the step read on the device
        self._graphed = None         # the GraphedTrainStep that has captured this optimizer's step (step() then raises)
        if device_schedule is not None:
            self._schedule_init(device_schedule)
        if model is not None:
            self.attach(model, grad_sync)

    # -- wiring -----------------------------------------------------------------------------------------------
    def attach(self, model: torch.nn.Module, grad_sync=None):
        enc = getattr(getattr(model, "bert", model), "encoder", None)
        if enc is None or not hasattr(enc, "grad_sink"):
            raise ValueError("AdamW.attach needs a mtvaf_amd model (TVNetSAModel2 / TVNetSAModel / BertModel)")
        if self.sam_rho > 0.0:
            self._sam_refuse_parallel(grad_sync)
        self._encoder = enc
        self._map_layers()
        # under GradSync the hook runs on the communication stream, where a slow update would delay the next layer's
        # all-reduce: full width there
        self._background_ok = grad_sync is None
        sink = enc.grad_sink
        sink.optimizer = self  # (a GradSync constructed later re-wires the hook through this, parallel.py)
        if self.accumulation_steps > 1:
            # fused accumulation: passes 1 .. k-1 add into the flat gradient buffers and report nothing; pass k reports every layer
            # with its complete gradient, so the in-backward update (overlap=True) and step() see final gradients only
            sink.accumulate_passes = self.accumulation_steps
            sink.reset_passes()
            if grad_sync is not None:
                grad_sync.accumulation_steps = self.accumulation_steps
        if self.overlap:
            sink.settle_params = True  # the hook's stream must also be behind the layer's last dX product (engine.py)
            if grad_sync is not None:
                grad_sync.adopt_optimizer(self)
            else:
                sink.on_layer_done = self._sink_hook
                sink.raw_stream_hook = True  # the update is one library launch on hip._st()
        return self

    def __repr__(self):
        return super().__repr__() + (f"\n(ema_decay: {self.ema_decay}, ema_warmup: {self.ema_warmup})" if self.ema_decay > 0.0 else "")

    def _sink_hook(self, li: int, flat):
        """GradSink.on_layer_done without data parallelism.  flat is None: the pass could not use the flat gradient buffers
        (some .grad pre-existed: gradient accumulation, or two encoder nodes under one backward) -- that layer is left to
        step(); but if an earlier pass has ALREADY updated layers from inside its backward, this pass accumulates on top of
        weights that moved mid-accumulation: refuse."""
        self.layer_pass_check(li, flat)
        if flat is not None:
            self._early_layer_update(li)

    def layer_pass_check(self, li: int, flat):
        if self.suspended or not self.overlap:
            return
        if flat is None and self._early:
            raise RuntimeError("mtvaf_amd.optim.AdamW(overlap=True): a second backward pass ran before optimizer.step() "
                               "(gradient accumulation needs overlap=False)")

    SEGMENT_PLANS = True  # (tests switch it off on an instance: layers with several groups then go tensor by tensor, as they used to)

    def _map_layers(self):
        """Every layer's plan: its parameter group (all 16 parameters in one: ``hip.adamw`` / ``hip.adamw_planes``), a list
        ``[(end element, group), ...]`` (several groups that one segmented launch can serve, ``layer_segments``), or None (tensor by
        tensor).  Groups are kept, not their values: ``group["lr"]`` is read at every update."""
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        self._layer_group = {}
        stores = None
        for li, layer in enumerate(self._encoder.layer):
            ps = layer.ordered_params()
            groups = [group_of.get(id(p)) for p in ps]
            plan = None
            if all(g is groups[0] for g in groups):
                plan = groups[0]
            elif self.SEGMENT_PLANS and all(g is not None for g in groups):
                if stores is None:
                    stores = self._encoder._prepare()[0]
                plan = layer_segments([stores[li].offsets[i] for i in range(len(ps))], [p.numel() for p in ps], groups,
                                      same=lambda a, b: a is b)
            self._layer_group[li] = plan

    def _plan(self, li: int, store):
        """The layer's plan (_map_layers); a segmented one only while it still describes the store's buffer."""
        plan = self._layer_group.get(li)
        if isinstance(plan, list) and plan[-1][0] != store.flat.numel():
            return None
        return plan

    def _layer_state(self, li: int, store):
        """Flat moment buffers of layer li; the per-parameter state entries are views of them."""
        key = ("layer", li)
        st = self._flat_state.get(key)
        if st is None or st["m"].numel() != store.flat.numel() or st["m"].device != store.flat.device:
            st = {"m": torch.zeros_like(store.flat), "v": torch.zeros_like(store.flat), "step": 0,
                  "step_t": torch.zeros((), dtype=torch.float32)}
            ema = self.ema_decay > 0.0
            if ema:
                st["ema"], st["ema_step"], st["ema_step_t"] = torch.zeros_like(store.flat), 0, torch.zeros((), dtype=torch.float32)
            if self.device_schedule is not None:  # one step count for everything: the layers share its two 0-dim tensors (host_step)
                st["step_t"] = self._sched_step_t
                if ema:
                    st["ema_step_t"] = self._sched_ema_step_t
            self._flat_state[key] = st
            steps, ema_steps = set(), set()
            for i, p in enumerate(self._encoder.layer[li].ordered_params()):
                off, n = store.offsets[i], p.numel()
                ps = self.state[p]
                m_v, v_v = st["m"][off:off + n].view(p.shape), st["v"][off:off + n].view(p.shape)
                if "exp_avg" in ps:  # per-parameter state that exists already (load_state_dict, or earlier per-tensor updates)
                    m_v.copy_(ps["exp_avg"])
                    v_v.copy_(ps["exp_avg_sq"])
                    steps.add(int(ps.get("step", 0)))
                ps["exp_avg"], ps["exp_avg_sq"] = m_v, v_v
                ps["step"] = st["step_t"]  # (torch.optim keeps `step` as a tensor too)
                if ema:
                    e_v = st["ema"][off:off + n].view(p.shape)
                    if "ema" in ps:
                        e_v.copy_(ps["ema"])
                    ema_steps.add(int(ps.get("ema_step", 0)) if "ema" in ps else 0)  # (a checkpoint without averages: they start now)
                    ps["ema"], ps["ema_step"] = e_v, st["ema_step_t"]
                self._param_layer[id(p)] = li
            if len(steps) > 1:
                raise RuntimeError(f"AdamW: the parameters of encoder layer {li} carry different step counts {sorted(steps)}")
            if len(ema_steps) > 1:
                raise RuntimeError(f"AdamW: the parameters of encoder layer {li} carry different EMA update counts {sorted(ema_steps)}")
            if steps:
                st["step"] = steps.pop()
                st["step_t"].fill_(st["step"])
            if ema_steps:
                st["ema_step"] = ema_steps.pop()
                st["ema_step_t"].fill_(st["ema_step"])
        return st

    def load_state_dict(self, state_dict):
        if self.sam_perturbed:
            raise RuntimeError("mtvaf_amd.optim.AdamW.load_state_dict: the weights are perturbed (perturb() without step()); call "
                               "step() or unperturb() first -- a checkpoint never holds the perturbed weights or their backup")
        super().load_state_dict(state_dict)
        # the flat per-layer buffers are rebuilt from the loaded per-parameter entries by the next _layer_state()
        self._flat_state = {}
        self._param_layer = {}
        self._early = set()
        if self.device_schedule is not None:
            counts = {int(s["step"]) for s in self.state.values() if "step" in s}
            if len(counts) > 1:
                raise RuntimeError(f"mtvaf_amd.optim.AdamW(device_schedule=...): the loaded parameters carry different step counts "
                                   f"{sorted(counts)}; the device keeps ONE counter for all of them")
            self._schedule_set_count(counts.pop() if counts else 0)

    # -- the schedule on the device --------------------------------------------------------------------
    def _schedule_init(self, table):
        who = "mtvaf_amd.optim.AdamW(device_schedule=...)"
        if not isinstance(table, ScheduleTable):
            raise TypeError(f"{who} takes what optim.schedule_table() returns")
        if self.overlap:
            raise ValueError(f"{who} needs overlap=False: updates enqueued from inside the backward pass run before step() has "
                             "advanced the device's step counter")
        if len(table.rows) < table.num_steps:
            raise ValueError(f"{who}: the table holds {len(table.rows)} rows, fewer than the {table.num_steps} steps it was built for")
        for g in self.param_groups:
            if tuple(float(b) for b in g["betas"]) != table.betas:
                raise ValueError(f"{who}: a parameter group has betas {tuple(g['betas'])}, the table was built for {table.betas} -- the "
                                 "bias corrections of a step are one row of the table, shared by every group")
        if self.ema_decay > 0.0 and (table.ema_decay, table.ema_warmup) != (self.ema_decay, self.ema_warmup):
            raise ValueError(f"{who}: the table was built for ema_decay={table.ema_decay}, ema_warmup={table.ema_warmup}, the optimizer "
                             f"averages with ema_decay={self.ema_decay}, ema_warmup={self.ema_warmup}")
        for g in self.param_groups:
            g.setdefault("initial_lr", g["lr"])  # the BASE lr the kernels multiply with the table's factor (a LambdaLR keeps it)
        self.device_schedule = table
        self._sched_count = 0      # the host mirror of the device counter: updates taken so far
        self._sched_dev = None     # {"table", "counter", "current"} on the device, made by the first step
        self._sched_states = []    # state dicts of the tensors the last launch updated one by one (host_step writes their counts)
        self._sched_step_t = torch.zeros((), dtype=torch.float32)      # state[p]["step"] of every encoder-layer parameter
        self._sched_ema_step_t = torch.zeros((), dtype=torch.float32)  # ... and state[p]["ema_step"]

    @property
    def schedule_count(self) -> int:
        """Updates taken so far under the device schedule (the host mirror of the device counter)."""
        return self._sched_count

    def _schedule_set_count(self, count: int):
        self._sched_count = int(count)
        self._sched_step_t.fill_(self._sched_count)
        self._sched_ema_step_t.fill_(self._sched_count)
        if self._sched_dev is not None:  # (in place: a captured graph holds the counter's address)
            self._sched_dev["counter"].fill_(self._sched_count)

    def _schedule_device(self, dev):
        d = self._sched_dev
        if d is None or d["counter"].device != dev:
            import numpy as np
            raw = torch.from_numpy(self.device_schedule.rows.view(np.uint8).copy())
            d = self._sched_dev = {"table": raw.to(dev), "counter": torch.full((1,), self._sched_count, dtype=torch.int64, device=dev),
                                   "current": torch.zeros(4, dtype=torch.int64, device=dev)}
        return d

    def _schedule_refuse_end(self):
        if self._sched_count + 1 > len(self.device_schedule.rows):
            raise RuntimeError(f"mtvaf_amd.optim.AdamW(device_schedule=...): update {self._sched_count + 1} lies past the end of the "
                               f"schedule table ({len(self.device_schedule.rows)} steps); nothing was launched")

    def assert_schedule_agrees(self):
        """``group["lr"]`` of every group is what the table gives the NEXT update (``initial_lr * factor(schedule_count)``): a
        scheduler that is stepped beside this optimizer for readers of ``group["lr"]`` has kept pace.  On demand, not per step."""
        f = self.device_schedule.lr_factors
        want = f[min(self._sched_count, len(f) - 1)]
        for i, g in enumerate(self.param_groups):
            if g["lr"] != g["initial_lr"] * want:
                raise AssertionError(f"parameter group {i}: lr {g['lr']!r} but the device schedule is at update {self._sched_count}, "
                                     f"lr {g['initial_lr'] * want!r}")

    def host_step(self):
        """The host's share of one update under the device schedule, and nothing else: the mirror of the device counter, the step
        and EMA counts ``state_dict()`` saves.  ``step()`` calls it behind its launches; a replay of a captured step calls it
        alone.  No launch, no synchronisation.  Raises before a step past the table's end."""
        self._schedule_refuse_end()
        c = self._sched_count = self._sched_count + 1
        ema_on = self.ema_decay > 0.0
        self._sched_step_t.fill_(c)  # (host tensors, shared by the parameters of every encoder layer)
        if ema_on:
            self._sched_ema_step_t.fill_(c)
        for st in self._flat_state.values():
            st["step"] = c
            if "ema" in st:
                st["ema_step"] = c
        for stt in self._sched_states:
            stt["step"] = c
            if ema_on:
                stt["ema_step"] = c

    def _schedule_count_check(self, what: str, step, ema_step):
        c = self._sched_count
        if int(step) != c or (ema_step is not None and int(ema_step) != c):
            raise RuntimeError(f"mtvaf_amd.optim.AdamW(device_schedule=...): {what} has taken {int(step)} updates"
                               + ("" if ema_step is None else f" ({int(ema_step)} of its average)")
                               + f", the schedule is at {c}: the device keeps ONE step counter (and one row of bias corrections and "
                               "EMA decay) for every parameter")

    def _schedule_launch(self, suppress: bool = False) -> bool:
        """Every launch of one update under the device schedule, on the current stream: the clip state (if wanted), the counter's
        advance, the ``*_sched`` updates.  No host value of the step enters a kernel argument, so a graph capture may contain the
        call.  ``suppress``: the warm-up of such a capture -- the advance is left out and the block's overrun word is raised instead,
        so every update kernel is loaded and every buffer allocated while nothing is written and no counter moves.
        -> False: no gradient, nothing launched."""
        self._refuse_swapped("step() was called")
        if not suppress:
            self._schedule_refuse_end()
        ema_on = self.ema_decay > 0.0
        layers, rest = self._collect()
        for li, _, store in layers:
            st = self._layer_state(li, store)
            self._schedule_count_check(f"encoder layer {li}", st["step"], st.get("ema_step"))
        group_jobs, states = {}, []  # id(group) -> (group, [(p, g, exp_avg, exp_avg_sq, ema), ...]); states: what host_step counts
        for group, p, g in rest:
            stt = self._tensor_state(p)
            if stt["step"] is not self._sched_step_t:  # (a view of a layer's flat state counts with the layer)
                self._schedule_count_check("a parameter", stt["step"], stt["ema_step"] if ema_on else None)
                states.append(stt)
            group_jobs.setdefault(id(group), (group, []))[1].append(
                (p, g, stt["exp_avg"], stt["exp_avg_sq"], stt["ema"] if ema_on else None))
        self._sched_states = states
        grads = [store.grad for _, _, store in layers] + [g for _, _, g in rest]
        if not grads:
            return False
        d = self._schedule_device(grads[0].device)
        clip = None
        if self.max_grad_norm > 0.0 or self.track_grad_norm:
            skipped = None if (not suppress or self.skipped_steps is None) else self.skipped_steps.clone()
            clip = self._clip_launch(grads)
            if suppress:  # (a warm-up pass is no step: its non-finite norm is not counted)
                self.skipped_steps.zero_() if skipped is None else self.skipped_steps.copy_(skipped)
        overrun = d["current"].view(torch.int32)[5:6]
        if suppress:
            overrun.fill_(1)
        else:
            hip.adamw_sched_advance(d["table"], d["counter"], d["current"])
        for li, plan, store in layers:
            self._update_layer(li, plan, store, clip=clip, current=d["current"], stamp=not suppress)
        for group, items in group_jobs.values():
            b1, b2 = group["betas"]
            hip.adamw_multi_sched([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items],
                                  group["initial_lr"], b1, b2, group["eps"], group["weight_decay"], d["current"], clip=clip,
                                  ema=[i[4] for i in items] if ema_on else None)
        if suppress:
            overrun.fill_(0)
        return True

    # -- averaged weights --------------------------------------------------------------------------------------------
    def _ema_omd(self, t: int) -> float:
        """1 - decay of EMA update t, in double: the C ABI rounds it to float once."""
        return float(1.0 - ema_decay_at(t, self.ema_decay, self.ema_warmup))

    def _ema_pairs(self):
        """-> (parameter side, average side): one pair per encoder layer whose flat buffers hold both, one per remaining tensor."""
        a, b, seen = [], [], set()
        enc = self._encoder
        if enc is not None and enc._stores is not None:
            for li, layer in enumerate(enc.layer):
                st, store = self._flat_state.get(("layer", li)), enc._stores[li]
                if st is None or "ema" not in st or not store.valid(layer) or st["ema"].numel() != store.flat.numel():
                    continue
                ps = layer.ordered_params()
                if all(self.state[p].get("ema") is not None and self.state[p]["ema"].data_ptr() == st["ema"].data_ptr() + 4 * store.offsets[i]
                       for i, p in enumerate(ps)):
                    a.append(store.flat)
                    b.append(st["ema"])
                    seen.update(id(p) for p in ps)
        for group in self.param_groups:
            for p in group["params"]:
                e = self.state[p].get("ema") if p in self.state else None
                if e is None or id(p) in seen:
                    continue
                if not p.is_contiguous() or not e.is_contiguous():
                    raise RuntimeError("non-contiguous parameter")
                seen.add(id(p))
                a.append(p.data)
                b.append(e)
        return a, b

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter the optimizer holds an average for with that average, bit for bit (one pair per encoder
        layer, the rest 48 pairs per launch), and declare the encoder's cached weight images stale.  A second call restores
        the training weights.  Until then ``ema_swapped`` is True and ``step()`` / the backward hook raise."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("mtvaf_amd.optim.AdamW.swap_ema: the optimizer keeps no averaged weights (ema_decay == 0)")
        if self._early:
            raise RuntimeError("mtvaf_amd.optim.AdamW.swap_ema: a backward pass has updated layers and optimizer.step() has not run yet")
        a, b = self._ema_pairs()
        hip.swap_f32(a, b)
        self.ema_swapped = not self.ema_swapped
        from . import engine
        engine.invalidate_weight_images()

    @contextlib.contextmanager
    def averaged_parameters(self):
        """``with optimizer.averaged_parameters(): evaluate(model)`` -- the averages swapped in for the block, the training
        weights back afterwards, also when the block raises."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self, model: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """``model.state_dict()`` with every parameter the optimizer averages replaced by (a copy of) its average: the model to
        ship.  Parameters without an average (frozen ones, the ResNet, anything no step has reached yet) and buffers keep their
        own values.  While the averages are swapped in the parameters ARE the averages, and that is what is returned."""
        out = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if self.ema_swapped:
            return out
        for name, p in model.named_parameters():
            e = self.state[p].get("ema") if p in self.state else None
            if e is not None and name in out and int(self.state[p].get("ema_step", 0)) > 0:
                out[name] = e.detach().clone().view(p.shape)
        return out

    def _refuse_swapped(self, what: str):
        if self.ema_swapped:
            raise RuntimeError(f"mtvaf_amd.optim.AdamW: {what} while the averaged weights are swapped in (swap_ema / "
                               "averaged_parameters): swap the training weights back first")

    # an update enqueued from inside the backward pass runs beside MFMA-bound products: on 128 blocks it trickles under
    # them (csrc/optim.hip); below this many token rows a layer's backward is shorter than such an update and it would
    # only pile up behind the pass
    BACKGROUND_MIN_ROWS = 2048
    BACKGROUND_BLOCKS = 128
    # (the pre-split path's second stream is lighter -- one grouped launch per layer -- and the update also writes the weights' plane
    # images: 256 blocks measured best there, 3257 - 3260 sentences/s against 3237 - 3238 at 128, 3220 - 3225 at 512, 3128 - 3133 at 64)
    BACKGROUND_BLOCKS_PLANES = 256
    # (bf16 mode below 4096 token rows -- C3: a layer's backward pass is 260 us, shorter than a 128-block trickle of its update --
    # 256 blocks: 5.52 - 5.54 -> 5.41 - 5.43 ms median step, same box; at 4864 rows (C4) 128 / 192 / 256 measure equal)
    BACKGROUND_BLOCKS_SHORT = 256
    BACKGROUND_SHORT_ROWS = 4096

    @staticmethod
    def _images(store, keep_read_mark: bool = False):
        """The image rule, once: -> (shadow, mats), the GEMM-operand image of the layer's weights that a kernel writing
        ``store.flat`` rewrites in the same pass.  ``shadow``: the bf16 image (bf16 compute mode, once a forward pass has built it);
        else ``mats``: the plane images of the four matrices (fp32 mode, pre-split operands) -- None as well when the buffer is no
        multiple of 4 elements, which the planes forms need.  At most one of the two is not None.

        The order and number of the two engine calls are part of the behaviour: ``planes_for_update`` is asked only where there is
        no shadow, exactly once per layer and writer, and it CLEARS the forward pass's read mark (and drops images no forward pass
        has read since the last update) unless ``keep_read_mark`` -- the writer the step's own update still follows (the SAM
        restore) passes it, so that the update finds the mark."""
        from . import engine
        shadow = engine.shadow_for_update(store.weights)
        mats = None
        if shadow is None:
            mats = engine.planes_for_update(store.weights, keep_read_mark=True) if keep_read_mark else engine.planes_for_update(store.weights)
        return shadow, (None if store.flat.numel() % 4 else mats)

    # the wrapper of mtvaf_amd.hip for a layer's one launch, by (plane images, segmented plan, device schedule)
    _LAYER_FORMS = {(planes, seg, sched): "adamw" + ("_planes" if planes else "") + ("_seg" if seg else "") + ("_sched" if sched else "")
                    for planes in (False, True) for seg in (False, True) for sched in (False, True)}

    def _update_layer(self, li: int, plan, store, *, clip=None, background: bool = False, rows: int = 0, current=None, stamp: bool = True):
        """The ONE launch that updates encoder layer ``li``.  ``current`` (the device schedule's block): the groups' BASE lr, no
        counter moves (``host_step`` does that).  Without it: the layer's step and EMA counters advance and lr / 1 - decay are the
        host's values of now.  ``stamp=False``: the images are not declared fresh (a launch that writes nothing)."""
        st = self._layer_state(li, store)
        sched = current is not None
        kw = dict(clip=clip)
        if sched:
            kw["ema"] = st.get("ema")
            lr_key, count = "initial_lr", current  # (the BASE lr: the kernel multiplies it with the block's factor)
        else:
            st["step"] += 1
            st["step_t"].fill_(st["step"])  # the 16 per-parameter state entries share this 0-dim tensor
            if "ema" in st:
                kw.update(ema=st["ema"], ema_omd=self._ema_omd(st["ema_step"]))
                st["ema_step"] += 1
                st["ema_step_t"].fill_(st["ema_step"])
            lr_key, count = "lr", st["step"]
        # a segmented plan ([(end element, group), ...]): lr and weight decay per segment, read now; betas and eps are the launch's
        segmented = isinstance(plan, list)
        group = plan[0][1] if segmented else plan
        b1, b2 = group["betas"]
        if segmented:
            hyper = ([(end, float(g[lr_key]), g["weight_decay"]) for end, g in plan], b1, b2, group["eps"], count)
        else:
            hyper = (float(group[lr_key]), b1, b2, group["eps"], group["weight_decay"], count)
        from . import engine
        shadow, mats = self._images(store)
        update = getattr(hip, self._LAYER_FORMS[mats is not None, segmented, sched])
        if mats is not None:
            # fp32 mode, pre-split operands: the weights' plane images are rewritten by the update kernel itself
            if not sched:
                kw["max_blocks"] = self.BACKGROUND_BLOCKS_PLANES if background else 0
            update(store.flat, store.grad, st["m"], st["v"], *hyper, mats, **kw)
            if stamp:
                engine.planes_written(store.weights)
            return
        if not sched:
            kw["max_blocks"] = ((self.BACKGROUND_BLOCKS_SHORT if 0 < rows < self.BACKGROUND_SHORT_ROWS else self.BACKGROUND_BLOCKS)
                                if background else 0)
        update(store.flat, store.grad, st["m"], st["v"], *hyper, p_bf16=shadow, **kw)  # (shadow: written in the same pass)
        if shadow is not None and stamp:
            engine.shadow_written(store.weights)
        engine.planes_rewrite(store.weights)  # (images exist but the fused form does not apply: rebuilt behind the update)

    def _early_layer_update(self, li: int):
        """Called from inside the backward pass (current stream: the one the layer's gradients are final on)."""
        stores = self._encoder._stores
        group = self._plan(li, stores[li]) if stores is not None else None
        if self.suspended or group is None or stores[li].grad is None:
            return
        self._refuse_swapped("a backward pass that updates the encoder layers (overlap=True) ran")
        if li in self._early:
            raise RuntimeError("mtvaf_amd.optim.AdamW(overlap=True): a second backward pass ran before optimizer.step()")
        # (the sink that is calling us: `encoder.grad_sink` would re-validate all twelve layer stores on each of the twelve calls --
        # 2304 pointer comparisons per step, 0.4 ms of host time in the launch-bound configurations)
        rows = getattr(self._encoder._sink, "token_rows", 0)
        # (layer 0 is the last one of the pass: nothing left to hide behind)
        background = self._background_ok and li > 0 and rows >= self.BACKGROUND_MIN_ROWS
        self._update_layer(li, group, stores[li], background=background, rows=rows)
        self._early.add(li)

    # -- sharpness-aware minimisation ---------------------------------------------------------------------
    def _sam_refuse_parallel(self, grad_sync=None):
        who = "mtvaf_amd.optim.AdamW(sam_rho > 0)"
        sink = getattr(self._encoder, "_sink", None) if self._encoder is not None else None
        owner = getattr(getattr(sink, "on_layer_done", None), "__self__", None)
        if grad_sync is None and type(owner).__name__ == "GradSync":
            grad_sync = owner
        several = grad_sync is not None and (getattr(grad_sync, "world", 1) > 1 or getattr(grad_sync, "force", False))
        try:
            import torch.distributed as dist
            several = several or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        except Exception:  # pragma: no cover
            pass
        if several:
            raise RuntimeError(f"{who}: data-parallel training (GradSync with several ranks) is not supported -- the perturbation "
                               "would be scaled by one rank's gradient norm; train on one GPU or build the optimizer with sam_rho=0")

    def _sam_buffer(self, key, like):
        b = self._sam_backup.get(key)
        if b is None or b.numel() != like.numel() or b.device != like.device:
            b = self._sam_backup[key] = torch.empty(like.numel(), dtype=torch.float32, device=like.device)
        return b

    @torch.no_grad()
    def perturb(self):
        """The ascent step of SAM, after the first backward pass: every parameter ``step()`` would update moves to
        ``p + sam_rho * g / (|g| + 1e-12)`` with ``|g|`` the global L2 norm of those gradients (double on the device, no host
        synchronisation), the weights it had are kept aside, and the first pass's gradients are discarded -- the second backward
        pass then leaves the gradient ``step()`` applies, after putting the weights back.  An encoder layer on the one-launch path
        is one launch that also rewrites the bf16 shadow or the plane images its GEMMs read, so the second forward pass multiplies
        by the perturbed weights.  A norm that is not finite leaves the weights alone and counts in ``sam_skipped``."""
        who = "mtvaf_amd.optim.AdamW.perturb"
        if self.sam_rho <= 0.0:
            raise RuntimeError(f"{who}: the optimizer was built with sam_rho=0; pass sam_rho > 0 to AdamW (or build_optimizer's args)")
        if self.sam_perturbed:
            raise RuntimeError(f"{who} was called twice without optimizer.step(): the weights are already perturbed (step() applies "
                               "the second pass's gradient and restores them; unperturb() only restores them)")
        self._refuse_swapped("perturb() was called")
        self._sam_refuse_parallel()
        if hip.STREAM_OVERRIDE is not None:
            raise RuntimeError(f"{who} was called from inside a backward hook -- the pass has not produced every gradient yet")
        layers, rest = self._collect()
        grads = [store.grad for _, _, store in layers] + [g for _, _, g in rest]
        if not grads:
            raise RuntimeError(f"{who}: no parameter has a gradient; call it after the first loss.backward()")
        partials, state, skipped = self._grad_sqnorm("sam", grads)
        hip.sam_finalize(partials, self.sam_rho, state, skipped)
        from . import engine
        jobs, fast = [], set()
        for li, _, store in layers:
            jobs.append((store, *self._images(store), self._sam_buffer(("layer", li), store.flat)))
            fast.add(li)
        enc = self._encoder
        stale = any(engine.images_left_stale(store.weights, shadow, mats) for store, shadow, mats, _ in jobs)
        if enc is not None and enc._stores is not None:  # (a layer that goes tensor by tensor below: nothing maintains its images)
            stale = stale or any(li not in fast and engine.images_left_stale(st.weights, None, None) for li, st in enumerate(enc._stores))
        if stale:
            engine.invalidate_weight_images()  # (before the stamps below)
        for store, shadow, mats, backup in jobs:
            if mats is not None:
                hip.sam_perturb_planes(store.flat, store.grad, backup, state, mats)
                engine.planes_written(store.weights, 0)  # (no optimizer step, no post-step hook: fresh as of now)
            else:
                hip.sam_perturb(store.flat, store.grad, backup, state, p_bf16=shadow)
                if shadow is not None:
                    engine.shadow_written(store.weights, 0)
        ps = [p.data for _, p, _ in rest]
        bs = [self._sam_buffer(id(p), p) for _, p, _ in rest]
        hip.sam_perturb_multi(ps, [g for _, _, g in rest], bs, state)
        self._sam_record = ([(store, backup) for store, _, _, backup in jobs], ps, bs)
        for group in self.param_groups:  # the first pass's gradients: the applied gradient is the second pass's alone
            for p in group["params"]:
                p.grad = None
        sink = getattr(enc, "_sink", None) if enc is not None else None
        if sink is not None:
            sink.reset_passes()
        self.sam_perturbed = True

    def _sam_restore(self, images: bool):
        """The weights of before ``perturb()`` back, bit for bit.  ``images``: through the forms that rewrite the bf16 shadow / the plane
        images from the restored values (an update that may write nothing follows, and stamps them); otherwise one multi-tensor copy
        (the update that follows rewrites them)."""
        layer_jobs, ps, bs = self._sam_record
        if not images:
            hip.sam_restore_multi([store.flat for store, _ in layer_jobs] + ps, [b for _, b in layer_jobs] + bs)
        else:
            for store, backup in layer_jobs:
                shadow, mats = self._images(store, keep_read_mark=True)
                if mats is not None:
                    hip.sam_restore_planes(store.flat, backup, mats)
                else:
                    hip.sam_restore(store.flat, backup, p_bf16=shadow)
            hip.sam_restore_multi(ps, bs)
        self._sam_record = None
        self.sam_perturbed = False

    @torch.no_grad()
    def unperturb(self):
        """Put back the weights of before ``perturb()`` without a step (the second pass raised, or its result is not wanted): one
        copy, and every cached weight image is declared stale -- the next forward pass rebuilds them."""
        if self.sam_perturbed:
            self._sam_restore(images=False)
            from . import engine
            engine.invalidate_weight_images()

    # -- the step ------------------------------------------------------------------------------------------------
    def _collect(self):
        """What a step updates right now, found ONCE for ``step()``, the device-schedule path and ``perturb()`` (so that all three
        mean the same tensors): -> (layers, rest).  ``layers``: ``(li, plan, store)`` of every encoder layer on the one-launch path
        -- it has a plan, its store is valid, and every parameter's ``.grad`` is its view of the store's flat gradient buffer.
        ``rest``: ``(group, parameter, contiguous gradient)`` of every other parameter with a gradient, in group order.  Layers a
        backward pass has already updated (``_early``; only with ``overlap=True``) are in neither.  Touches no optimizer state and no
        counter; what happens with the result is the caller's."""
        done, layers = set(), []
        enc = self._encoder
        if enc is not None and enc._stores is not None:
            if len(self._layer_group) != len(enc.layer):
                self._map_layers()
            for li, layer in enumerate(enc.layer):
                ps = layer.ordered_params()
                if li in self._early:
                    done.update(id(p) for p in ps)
                    continue
                store = enc._stores[li]
                plan = self._plan(li, store)
                if plan is None or store.grad is None or not store.valid(layer):
                    continue
                lo = store.grad.data_ptr()
                if all(p.grad is not None and p.grad.data_ptr() == lo + 4 * store.offsets[i] and p.grad.is_contiguous()
                       for i, p in enumerate(ps)):
                    layers.append((li, plan, store))
                    done.update(id(p) for p in ps)
        rest = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None or id(p) in done:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("mtvaf_amd.optim.AdamW updates dense fp32 parameters on the MI355X only")
                if not p.is_contiguous():
                    raise RuntimeError("non-contiguous parameter")
                rest.append((group, p, p.grad if p.grad.is_contiguous() else p.grad.contiguous()))
        return layers, rest

    def _tensor_state(self, p):
        """``state[p]`` of a tensor updated on its own, its moments (and average) made at the first update."""
        stt = self.state[p]
        if "exp_avg" not in stt:
            stt["exp_avg"], stt["exp_avg_sq"], stt["step"] = torch.zeros_like(p), torch.zeros_like(p), 0
        if self.ema_decay > 0.0 and "ema" not in stt:  # (with exp_avg, or behind a checkpoint written without averages: they start now)
            stt["ema"], stt["ema_step"] = torch.zeros_like(p), 0
        return stt

    _NORM_ATTRS = {"clip": ("_clip_state", "last_grad_norm", "skipped_steps", "_clip_partials"),
                   "sam": ("_sam_state", "last_sam_norm", "sam_skipped", "_sam_partials")}

    def _grad_sqnorm(self, which: str, grads):
        """The device norm state of clipping ("clip") or of perturb() ("sam") -- 4 floats a finalize kernel writes, a 0-dim view of
        the norm in them, an int32 counter of non-finite norms, doubles for the partial sums: made on the gradients' device, the
        partials grown as needed -- and the sums of squares of ``grads`` launched into it.
        -> (partial sums, state, counter): what ``hip.grad_clip_finalize`` / ``hip.sam_finalize`` take."""
        s_state, s_norm, s_count, s_part = self._NORM_ATTRS[which]
        dev = grads[0].device
        state = getattr(self, s_state)
        if state is None or state.device != dev:
            state = torch.zeros(4, dtype=torch.float32, device=dev)
            setattr(self, s_state, state)
            setattr(self, s_norm, state[0])
            setattr(self, s_count, torch.zeros((), dtype=torch.int32, device=dev))
            setattr(self, s_part, None)
        slots = hip.grad_sqnorm_slots(grads)
        partials = getattr(self, s_part)
        if partials is None or partials.numel() < slots:
            partials = torch.empty(slots, dtype=torch.float64, device=dev)
            setattr(self, s_part, partials)
        return hip.grad_sqnorm(grads, partials), state, getattr(self, s_count)

    def _clip_launch(self, grads):
        """Norm + finalize over the gradients this step applies, on the stream of the updates that follow; -> the device state."""
        partials, state, skipped = self._grad_sqnorm("clip", grads)
        return hip.grad_clip_finalize(partials, self.max_grad_norm, state, skipped, self.skip_nonfinite)

    def _new_accumulation(self):
        sink = getattr(self._encoder, "_sink", None) if self._encoder is not None else None
        if sink is not None and sink.accumulate_passes:
            sink.reset_passes()

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        self._new_accumulation()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._new_accumulation()
        self._refuse_swapped("step() was called")
        clipping = self.max_grad_norm > 0.0 or self.track_grad_norm
        ema_on = self.ema_decay > 0.0
        if self.sam_perturbed:
            # the weights of before perturb() first.  Where the update below may write nothing (a non-finite norm under clipping) the
            # images it stamps fresh must already hold the restored values; otherwise it rewrites them itself and a copy is enough
            self._sam_restore(images=clipping and self.skip_nonfinite)
        if clipping and hip.STREAM_OVERRIDE is not None:
            raise RuntimeError("mtvaf_amd.optim.AdamW: step() with max_grad_norm / track_grad_norm was called from inside a backward "
                               "hook -- the gradient norm would be taken before the pass has produced every gradient")
        if self.device_schedule is not None:
            if self._graphed is not None:
                raise RuntimeError("mtvaf_amd.optim.AdamW: step() was called, but this optimizer's step is part of a captured "
                                   "GraphedTrainStep -- every call of that object IS the step (close() it to step eagerly again)")
            if self._schedule_launch():
                self.host_step()
            return loss
        layers, rest = self._collect()
        self._early = set()
        touched = set()  # layers updated tensor by tensor this step: ONE step counter per layer, shared with the flat path
        # (id(group), step number, EMA update number) -> (group, [(p, g, exp_avg, exp_avg_sq, ema), ...]): one launch per 48 tensors each
        group_jobs: Dict[tuple, tuple] = {}
        for group, p, g in rest:
            stt = self._tensor_state(p)
            li = self._param_layer.get(id(p))
            fst = self._flat_state.get(("layer", li)) if li is not None else None
            ema_no = -1
            if fst is not None and stt["step"] is fst["step_t"]:
                # moments live in the layer's flat buffers (views): this tensor-by-tensor update advances the layer's counter
                step_no = fst["step"] + 1
                if ema_on:
                    ema_no = fst["ema_step"]
                touched.add(li)
            else:
                if torch.is_tensor(stt["step"]):
                    stt["step"] = int(stt["step"])
                stt["step"] += 1
                step_no = stt["step"]
                if ema_on:
                    ema_no = stt["ema_step"] = int(stt["ema_step"])
                    stt["ema_step"] += 1
            group_jobs.setdefault((id(group), step_no, ema_no), (group, []))[1].append(
                (p, g, stt["exp_avg"], stt["exp_avg_sq"], stt["ema"] if ema_on else None))
        clip = None
        if clipping:
            # every gradient about to be applied, each once: a layer's flat gradient buffer stands for its 16 views.  The launches
            # go to the stream of the updates below, behind the producers of every gradient
            grads = [store.grad for _, _, store in layers] + [g for _, _, g in rest]
            if grads:
                clip = self._clip_launch(grads)
        for li, plan, store in layers:
            self._update_layer(li, plan, store, clip=clip)
        for (_, step_no, ema_no), (group, items) in group_jobs.items():
            b1, b2 = group["betas"]
            hip.adamw_multi([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items],
                            float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], step_no, clip=clip,
                            **(dict(ema=[i[4] for i in items], ema_omd=self._ema_omd(ema_no)) if ema_on else {}))
        for li in touched:
            fst = self._flat_state[("layer", li)]
            fst["step"] += 1
            fst["step_t"].fill_(fst["step"])
            if ema_on:
                fst["ema_step"] += 1
                fst["ema_step_t"].fill_(fst["ema_step"])
        return loss


def _is_layer_mix(name: str) -> bool:
    """The two parameters of a model's `LayerMix` (args.layer_mix): softmax logits and one scale, never weight-decayed."""
    return name.startswith("layer_mix.") or ".layer_mix." in name


def _is_mlm_head(name: str) -> bool:
    """A parameter of a model's `MaskedLMHead` (args.mlm_head) under its own name.  The tied word table is not one: it is listed
    once, under the encoder's name, and trains with the encoder."""
    return name.startswith("mlm_head.") or ".mlm_head." in name


def _mlm_no_decay(name: str) -> bool:
    """... exempt from weight decay whatever ``no_decay`` names: its LayerNorm, the dense bias and the vocabulary bias."""
    return _is_mlm_head(name) and (name.endswith(".bias") or "LayerNorm." in name or "layer_norm." in name)


def reference_param_groups(model: torch.nn.Module, lr: float, use_prefix: bool = True) -> List[Dict]:
    """The parameter groups of modules/train.py:887-916 (by parameter name, in the reference's order).  A model with args.layer_mix
    (not the reference's) gets one more group behind them: the mix's two parameters, at the head's lr (``lr`` without a prefix),
    weight decay 0.  A model with args.mlm_head (not the reference's either): the head's dense weight (and an untied decoder) join
    the head group, its LayerNorm and biases the weight-decay-0 group behind it (shared with the mix)."""
    named = list(model.named_parameters())
    mix = [p for n, p in named if _is_layer_mix(n) or _mlm_no_decay(n)]
    named = [(n, p) for n, p in named if not (_is_layer_mix(n) or _mlm_no_decay(n))]
    if not use_prefix:  # bert_before_train: every parameter, one group
        return [{"params": [p for _, p in named], "lr": lr}] + ([{"params": mix, "lr": lr, "weight_decay": 0.0}] if mix else [])
    groups = [
        {"lr": lr, "weight_decay": 1e-2, "params": [p for n, p in named if "bert" in n]},
        {"lr": lr, "weight_decay": 1e-2, "params": [p for n, p in named if "encoder_conv" in n or "gates" in n]},
        {"lr": 5e-2, "weight_decay": 1e-2, "params": [p for n, p in named if "crf" in n or n.startswith("fc") or _is_mlm_head(n)]},
    ]
    if mix:
        groups.append({"lr": 5e-2, "weight_decay": 0.0, "params": mix})
    return groups


DEFAULT_NO_DECAY = ("bias", "LayerNorm.weight")


def finetune_param_groups(model: torch.nn.Module, lr: float, weight_decay: float = 1e-2, no_decay=DEFAULT_NO_DECAY,
                          layer_lr_decay: float = 1.0, head_lr: float = 5e-2, use_prefix: bool = True) -> List[Dict]:
    """The usual BERT fine-tuning recipe on the reference's name partition (new functionality: the reference trains with one weight
    decay everywhere and one lr per group, modules/train.py:894-916).

    The partition by name is ``reference_param_groups``'s -- ``bert*``; ``encoder_conv*`` / ``gates*``; ``crf*`` / ``fc*`` at
    ``head_lr``; with the quirk that ``projectors.*`` / ``*img_classifier.*`` match no group; ``use_prefix=False``: every parameter,
    one partition.  Then
      * every partition is split by the ``no_decay`` name test (a parameter whose name contains one of the strings gets weight
        decay 0, the others ``weight_decay``), and
      * the encoder is split by depth: layer ``l`` of ``L`` (``encoder.layer.<l>.``) trains at ``lr * layer_lr_decay ** (L - 1 - l)``,
        the embeddings at ``lr * layer_lr_decay ** L``, whatever sits above the last layer (the pooler) at ``lr``.
    The two parameters of a `LayerMix` (``layer_mix.scalars``, ``layer_mix.gamma``; args.layer_mix) belong to the head partition and
    are always exempt from weight decay, whatever ``no_decay`` names.  So do the parameters of a `MaskedLMHead` (``mlm_head.*``;
    args.mlm_head): the dense weight (and an untied decoder) with weight decay, the LayerNorm and the biases always without; the
    tied word table is the encoder's.
    Groups come in the order their first parameter has in ``named_parameters()``.  With ``no_decay=()`` and ``layer_lr_decay=1`` these
    are the reference groups.  An encoder layer then holds two groups; ``AdamW`` still updates it with one launch (``layer_segments``)."""
    import re
    named = list(model.named_parameters())
    no_decay = tuple(no_decay or ())
    if use_prefix:
        parts = [(lr, [(n, p) for n, p in named if "bert" in n], True),
                 (lr, [(n, p) for n, p in named if "encoder_conv" in n or "gates" in n], False),
                 (head_lr, [(n, p) for n, p in named if "crf" in n or n.startswith("fc") or _is_layer_mix(n) or _is_mlm_head(n)], False)]
    else:
        parts = [(lr, named, True)]
    layer_of = lambda n: re.search(r"encoder\.layer\.(\d+)\.", n)
    L = 1 + max((int(layer_of(n).group(1)) for n, _ in named if layer_of(n)), default=-1)
    groups = []
    for base_lr, items, by_depth in parts:
        split: Dict[tuple, list] = {}
        for n, p in items:
            power = 0
            if by_depth and layer_lr_decay != 1.0:
                power = L - 1 - int(layer_of(n).group(1)) if layer_of(n) else (L if "embeddings." in n else 0)
            split.setdefault((power, any(s in n for s in no_decay) or _is_layer_mix(n) or _mlm_no_decay(n)), []).append(p)
        if not split:  # (the reference keeps its empty second group too)
            split[(0, False)] = []
        groups.extend({"lr": base_lr * layer_lr_decay ** power, "weight_decay": 0.0 if exempt else weight_decay, "params": ps}
                      for (power, exempt), ps in split.items())
    return groups


def linear_warmup_factor(num_warmup_steps: float, num_training_steps: int):
    """The lr factor of ``linear_schedule_with_warmup`` as a function of the step (what ``schedule_table`` tabulates)."""

    def factor(step: int) -> float:
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))

    return factor


def linear_schedule_with_warmup(optimizer, num_warmup_steps: float, num_training_steps: int):
    """transformers.get_linear_schedule_with_warmup restated (the reference passes a float warm-up count,
    train.py:922-924): lr factor = step / warmup while warming up, then linear decay to 0."""
    return torch.optim.lr_scheduler.LambdaLR(optimizer, linear_warmup_factor(num_warmup_steps, num_training_steps))


def accumulation_plan(args):
    """-> (overlap, fused accumulation steps): the ONE rule that picks how ``build_optimizer`` trains the encoder under
    ``args.gradient_accumulation_steps`` (train.py:616-625 steps every `accum` backward passes).

    * accum == 1: layers are updated from inside the backward pass (overlap) unless ``args.overlap_optimizer`` is off or a global
      gradient norm is wanted (it exists only once the whole backward pass has ended: clipping / tracking step after it).
    * accum > 1 without ``args.fused_accumulation``: (False, 1) -- the fallback: fresh gradient tensors per micro-batch, autograd adds
      them, ``step()`` updates.
    * accum > 1 with ``args.fused_accumulation``: (overlap under the conditions above, accum) -- the micro-batches add into the
      encoder's flat gradient buffers and, with overlap, the last one updates each layer from inside its backward
      (``AdamW(accumulation_steps=accum)``)."""
    accum = int(getattr(args, "gradient_accumulation_steps", 1) or 1)
    max_grad_norm = float(getattr(args, "max_grad_norm", 0.0) or 0.0)
    fused = bool(getattr(args, "fused_accumulation", False)) and accum > 1
    overlap = (bool(getattr(args, "overlap_optimizer", True)) and (accum == 1 or fused)
               and not (max_grad_norm > 0.0 or bool(getattr(args, "track_grad_norm", False))))
    return overlap, (accum if fused else 1)


def build_optimizer(model: torch.nn.Module, args, train_num_steps: int):
    """-> (optimizer, scheduler) as SATrainer2.train() sets them up (train.py:574-578, 887-926)."""
    use_prefix = bool(getattr(args, "use_prefix", False))
    # the fine-tuning recipe (not the reference's): args.no_decay -- False (default), True (DEFAULT_NO_DECAY) or a tuple of name
    # fragments whose parameters get weight decay 0 -- and args.layer_lr_decay (1.0: one lr for the whole encoder)
    no_decay = getattr(args, "no_decay", False)
    no_decay = DEFAULT_NO_DECAY if no_decay is True else tuple(no_decay or ())
    layer_lr_decay = float(getattr(args, "layer_lr_decay", 1.0) or 1.0)
    if no_decay or layer_lr_decay != 1.0:
        groups = finetune_param_groups(model, args.lr, no_decay=no_decay, layer_lr_decay=layer_lr_decay, use_prefix=use_prefix)
    else:
        groups = reference_param_groups(model, args.lr, use_prefix)
    if use_prefix:
        for n, p in model.named_parameters():  # freeze resnet (:920-921)
            if "image_model" in n:
                p.requires_grad = False
    on_gpu = any(p.is_cuda for g in groups for p in g["params"])
    number = lambda name, default=0.0: float(getattr(args, name, default) or default)
    max_grad_norm = number("max_grad_norm")  # 0: unchanged, the reference does not clip (train.py:620-625)
    track_grad_norm = bool(getattr(args, "track_grad_norm", False))
    ema_decay = number("ema_decay")  # 0: unchanged, the reference keeps no averaged weights
    ema_warmup = bool(getattr(args, "ema_warmup", True))
    # args.device_schedule (default off): lr factor, bias corrections and EMA decay of every step as a table on the device, read by
    # the *_sched kernels -- the optimizer step can then be captured (GraphedTrainStep(model, batch, optimizer=opt)); updates after
    # the backward pass (overlap=False), and the scheduler returned only mirrors the table for readers of group["lr"]
    device_schedule = bool(getattr(args, "device_schedule", False))
    # args.adv_eps > 0 (default 0: nothing changes): adversarial training on the embedding output (mtvaf_amd.adversarial,
    # DESIGN.md 4.23; args.adv_norm, args.adv_steps, args.adv_weight).  args.sam_rho > 0 (default 0: nothing changes):
    # sharpness-aware minimisation
    adv_eps, sam_rho = number("adv_eps"), number("sam_rho")
    accum = int(getattr(args, "gradient_accumulation_steps", 1) or 1)
    grad_sync = getattr(args, "grad_sync", None)
    warmup_steps = getattr(args, "warmup_ratio", 0.01) * train_num_steps
    if device_schedule and not on_gpu:
        raise ValueError("build_optimizer: device_schedule is implemented by the gfx950 AdamW kernels; the model is not on the GPU")
    if on_gpu:
        # the path's own optimizer kernels.  Updates from inside the backward pass only when every backward is followed by a
        # step (gradient_accumulation_steps == 1: train.py:616-625 steps every `accum` backward passes)
        overlap, fused_steps = accumulation_plan(args)
        # One adversarial step is 1 + adv_steps backward passes: on the fallback the update waits for step(); with
        # args.fused_accumulation they are the passes of the fused accumulation.  The Adversary is left in `optimizer.adversary`;
        # the trainer calls its step(**batch) in place of model(**batch).loss.backward()
        adv_passes = 1 + int(getattr(args, "adv_steps", 1) or 1) if adv_eps > 0.0 else 0
        if adv_passes:
            if accum > 1:
                raise ValueError("build_optimizer: adv_eps > 0 with gradient_accumulation_steps > 1 is not supported")
            if grad_sync is not None or device_schedule:
                raise ValueError("build_optimizer: adv_eps > 0 is single-GPU and eager (no grad_sync, no device_schedule)")
            if bool(getattr(args, "fused_accumulation", False)):
                fused_steps = adv_passes  # (overlap stays what the plan gave a step of one micro-batch)
            else:
                overlap = False
        extra = {"accumulation_steps": fused_steps} if fused_steps > 1 else {}
        # Under SAM the update waits for step(), as under clipping; the trainer calls
        # mtvaf_amd.sam.SharpnessAware(model, opt).step(**batch) in place of its three lines
        if sam_rho > 0.0:
            if accum > 1 or adv_passes:
                raise ValueError("build_optimizer: sam_rho > 0 with gradient_accumulation_steps > 1 or adv_eps > 0 is not supported")
            if grad_sync is not None or device_schedule:
                raise ValueError("build_optimizer: sam_rho > 0 is single-GPU and eager (no grad_sync, no device_schedule)")
            overlap = False
            extra["sam_rho"] = sam_rho
        if device_schedule:
            overlap = False
            extra["device_schedule"] = schedule_table(linear_warmup_factor(warmup_steps, train_num_steps), train_num_steps,
                                                      (0.9, 0.999), ema_decay, ema_warmup)  # (AdamW's default betas, as below)
        opt = AdamW(groups, lr=args.lr, model=model, overlap=overlap, grad_sync=grad_sync, max_grad_norm=max_grad_norm,
                    track_grad_norm=track_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup, **extra)
        if adv_passes:
            from .adversarial import from_args
            opt.adversary = from_args(model, args, optimizer=opt)
        if device_schedule:
            return opt, ScheduleMirror(opt)
    else:
        if max_grad_norm > 0.0:
            raise ValueError("build_optimizer: max_grad_norm is implemented by the gfx950 AdamW kernels; the CPU fallback "
                             "(torch.optim.AdamW) would ignore it -- clip with torch.nn.utils.clip_grad_norm_ there")
        if ema_decay > 0.0:
            raise ValueError("build_optimizer: ema_decay is implemented by the gfx950 AdamW kernels; the CPU fallback "
                             "(torch.optim.AdamW) would ignore it")
        if adv_eps > 0.0:
            raise ValueError("build_optimizer: adv_eps is implemented by the gfx950 kernels; the model is not on the GPU")
        if sam_rho > 0.0:
            raise ValueError("build_optimizer: sam_rho is implemented by the gfx950 AdamW kernels; the model is not on the GPU")
        opt = torch.optim.AdamW(groups, lr=args.lr)
    sched = linear_schedule_with_warmup(opt, warmup_steps, train_num_steps)
    return opt, sched
