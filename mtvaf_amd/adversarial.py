"""Adversarial training on the embedding output: FGM (Miyato et al. 2017), PGD and FreeLB-style averaged steps (Zhu et al. 2020)
for ``TVNetSAModel2`` and ``TVNetSAModel`` -- new functionality, the reference trainer has no adversarial step (DESIGN.md
section 4.23).

    adv = Adversary(model, eps=1.0)            # FGM: one clean pass, one perturbed pass
    res = adv.step(**batch)                    # in place of  model(**batch).loss.backward()
    optimizer.step(); optimizer.zero_grad()

The perturbation is made by one kernel call per pass (``hip.adv_perturb``, csrc/adversarial.hip) from the gradient that
``engine.EmbeddingTapFunction`` keeps at the embedding seam (``BertModel.embedding_tap``); nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import engine, hip


class Adversary:
    """``eps``: radius of the ball; ``norm``: "l2" or "linf"; ``scope``: "sentence" (one ball over all unmasked tokens of a
    sentence) or "token" (one per token); ``steps``: perturbed passes per step (1 = FGM); ``step_size``: the ascent step of every
    pass when ``steps > 1`` (default ``eps / steps``; the first pass starts from 0, so its perturbation has that norm); ``weight``:
    weight of the adversarial loss -- each perturbed pass is backpropagated with ``weight / steps``.

    ``optimizer``: the optimizer that will apply the step, if it is a ``mtvaf_amd.optim.AdamW``.  By default every backward pass of
    ``step`` takes the encoder's fallback (fresh gradient tensors, autograd adds them).  An optimizer built with
    ``accumulation_steps = 1 + steps`` (fused accumulation) makes the passes add into the flat gradient buffers, and
    with ``overlap=True`` the last pass updates the layers from inside its backward.  Any other ``accumulation_steps > 1``, or
    ``overlap=True`` without that count (the clean pass would move the weights under the perturbed one), is a ``ValueError``.
    Data parallelism (``GradSync``, several ranks) and a captured step (``GraphedTrainStep``) are refused with a ``RuntimeError``."""

    def __init__(self, model: torch.nn.Module, eps: float = 1.0, norm: str = "l2", scope: str = "sentence", steps: int = 1,
                 step_size=None, weight: float = 1.0, optimizer=None):
        bert = getattr(model, "bert", None)
        if bert is None or not hasattr(bert, "embedding_tap"):
            raise ValueError("Adversary needs a mtvaf_amd model with a `bert` encoder (TVNetSAModel2 / TVNetSAModel)")
        eps, weight, steps = float(eps), float(weight), int(steps)
        if not (eps > 0.0) or eps == float("inf"):
            raise ValueError(f"Adversary: eps must be a positive finite radius, got {eps}")
        if norm not in hip.ADV_NORMS or scope not in hip.ADV_SCOPES:
            raise ValueError(f"Adversary: norm {norm!r} / scope {scope!r}: expected one of {sorted(hip.ADV_NORMS)} / "
                             f"{sorted(hip.ADV_SCOPES)}")
        if steps < 1:
            raise ValueError("Adversary: steps must be >= 1")
        step_size = eps / steps if step_size is None else float(step_size)
        if not (step_size > 0.0) or step_size == float("inf"):
            raise ValueError(f"Adversary: step_size must be positive and finite, got {step_size}")
        if not (weight >= 0.0):
            raise ValueError(f"Adversary: weight must be >= 0, got {weight}")
        self.model, self.bert = model, bert
        self.eps, self.norm, self.scope, self.steps, self.step_size, self.weight = eps, norm, scope, steps, step_size, weight
        self.optimizer = optimizer
        if optimizer is not None:
            self._check_optimizer(optimizer)

    @property
    def passes(self) -> int:
        """Backward passes of one ``step``: the clean one and ``steps`` perturbed ones."""
        return 1 + self.steps

    def _check_optimizer(self, opt):
        acc = int(getattr(opt, "accumulation_steps", 1) or 1)
        if acc != 1 and acc != self.passes:
            raise ValueError(f"Adversary(steps={self.steps}) runs {self.passes} backward passes per step, but the optimizer was built "
                             f"with accumulation_steps={acc}: build it with accumulation_steps={self.passes} (fused accumulation) or "
                             "1 (the fallback)")
        if getattr(opt, "overlap", False) and acc != self.passes:
            raise ValueError(f"Adversary: AdamW(overlap=True) would update the encoder from inside the clean pass's backward; build it "
                             f"with accumulation_steps={self.passes} or overlap=False")
        if getattr(opt, "_graphed", None) is not None:
            raise RuntimeError("Adversary: this optimizer's step is part of a captured GraphedTrainStep; an adversarial step is "
                               "several eager passes and is not captured")

    def _check_sink(self):
        """What only shows once the encoder has its gradient sink: the hook of a GradSync, an optimizer attached without a word
        to this object, several ranks."""
        sink = getattr(self.bert.encoder, "_sink", None)
        if sink is not None:
            owner = getattr(sink.on_layer_done, "__self__", None)
            if owner is not None and type(owner).__name__ == "GradSync":
                raise RuntimeError("Adversary: data-parallel training (GradSync) is not supported")
            if sink.optimizer is not None and sink.optimizer is not self.optimizer:
                self._check_optimizer(sink.optimizer)
            if sink.accumulate_passes not in (0, 1, self.passes):
                raise ValueError(f"Adversary(steps={self.steps}) runs {self.passes} backward passes per step, but the encoder "
                                 f"accumulates over {sink.accumulate_passes}")
        if self.optimizer is not None:
            self._check_optimizer(self.optimizer)
        try:
            import torch.distributed as dist
            several = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        except Exception:  # pragma: no cover
            several = False
        if several:
            raise RuntimeError("Adversary: data-parallel training (several ranks) is not supported")

    def step(self, **batch) -> Dict[str, torch.Tensor]:
        """The backward passes of one training step on ``batch`` (the keyword arguments of ``model.forward``, labels included):
        a clean pass, then ``steps`` passes on ``embeddings + delta``; every pass computes the visual prompt and draws its dropout
        masks anew.  The caller then calls ``optimizer.step()``.  -> ``loss`` (clean, detached), ``adv_loss`` (mean of the perturbed
        passes' losses, detached), ``logits`` (clean pass), ``grad_norm`` / ``delta_norm`` [B] (the last kernel call's per-sentence
        norms of the gradient and of the perturbation), ``nonfinite`` (0-dim: sentences whose gradient norm was inf / NaN in any
        call -- their perturbation took no gradient term).  After a ``step`` that raised, clear the gradients
        (``optimizer.zero_grad()``) before the next one."""
        self._check_sink()
        mask = batch.get("attention_mask")
        if mask is None:
            raise ValueError("Adversary.step needs attention_mask: it marks the rows the perturbation covers")
        bert = self.bert
        if bert.embedding_tap is not None:
            raise RuntimeError("Adversary.step: the encoder's embedding_tap is already in use")
        tap = engine.EmbeddingTap(capture=True)
        bert.embedding_tap = tap
        try:
            clean = self.model(**batch)
            if clean.loss is None:
                raise ValueError("Adversary.step needs a batch with labels: the clean pass returned no loss")
            clean.loss.backward()
            m8 = hip.adv_mask(mask)
            first = self.eps if self.steps == 1 else min(self.step_size, self.eps)
            delta, stats, nonfinite, adv_loss = None, None, None, None
            for k in range(1, self.steps + 1):
                g, tap.grad = tap.grad, None
                if g is None:
                    raise RuntimeError("Adversary.step: no gradient reached the embedding output (is the encoder frozen?)")
                delta, _, stats = hip.adv_perturb(g.contiguous(), m8, first if k == 1 else self.eps, self.step_size, self.norm,
                                                  self.scope, delta_in=delta)
                bad = (~torch.isfinite(stats[:, 0])).sum()
                nonfinite = bad if nonfinite is None else nonfinite + bad
                tap.delta, tap.capture = delta, k < self.steps
                loss_k = self.model(**batch).loss
                (loss_k * (self.weight / self.steps)).backward()
                adv_loss = loss_k.detach() if adv_loss is None else adv_loss + loss_k.detach()
        finally:
            bert.embedding_tap = None
        return {"loss": clean.loss.detach(), "adv_loss": adv_loss / self.steps, "logits": clean.logits, "grad_norm": stats[:, 0],
                "delta_norm": stats[:, 1], "nonfinite": nonfinite}


def from_args(model: torch.nn.Module, args, optimizer=None):
    """-> the ``Adversary`` that ``args`` asks for, or None at the default ``args.adv_eps = 0``: ``adv_eps`` (radius), ``adv_norm``
    ("l2"), ``adv_scope`` ("sentence"), ``adv_steps`` (1), ``adv_step_size`` (None: eps / steps), ``adv_weight`` (1.0)."""
    eps = float(getattr(args, "adv_eps", 0.0) or 0.0)
    if eps <= 0.0:
        return None
    return Adversary(model, eps=eps, norm=getattr(args, "adv_norm", "l2") or "l2", scope=getattr(args, "adv_scope", "sentence") or "sentence",
                     steps=int(getattr(args, "adv_steps", 1) or 1), step_size=getattr(args, "adv_step_size", None),
                     weight=float(getattr(args, "adv_weight", 1.0)), optimizer=optimizer)
