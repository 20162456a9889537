"""Sharpness-aware minimisation (SAM, Foret et al. 2021; the fine-tuning scene's "AWP" in its global form) for ``TVNetSAModel2``
and ``TVNetSAModel`` -- new functionality, the reference trainer has nothing like it.

    opt = AdamW(groups, lr=..., model=model, sam_rho=0.05)       # or build_optimizer(model, args, steps) with args.sam_rho
    sam = SharpnessAware(model, opt)
    res = sam.step(**batch)                                       # in place of  backward / optimizer.step() / zero_grad()

The ascent step, the restore and everything the weight-image cache needs to hear about them are ``AdamW.perturb()`` and
``AdamW.step()`` (mtvaf_amd/optim.py, csrc/optim.hip); this module is the loop around them.  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Dict

import torch


class SharpnessAware:
    """``optimizer``: a ``mtvaf_amd.optim.AdamW`` built with ``sam_rho > 0`` and attached to ``model`` (``model=`` at construction,
    or ``attach``).  What that optimizer refuses -- ``overlap=True``, ``accumulation_steps > 1``, a device schedule, a ``GradSync``
    with several ranks -- it has refused when it was built."""

    def __init__(self, model: torch.nn.Module, optimizer):
        from .optim import AdamW
        if not isinstance(optimizer, AdamW) or optimizer.sam_rho <= 0.0:
            raise ValueError("SharpnessAware needs a mtvaf_amd.optim.AdamW built with sam_rho > 0 (the ascent step and the restore are "
                             "its perturb() and step())")
        enc = getattr(getattr(model, "bert", model), "encoder", None)
        if enc is None or not hasattr(enc, "grad_sink"):
            raise ValueError("SharpnessAware needs a mtvaf_amd model (TVNetSAModel2 / TVNetSAModel)")
        if optimizer._encoder is None:
            optimizer.attach(model)
        elif optimizer._encoder is not enc:
            raise ValueError("SharpnessAware: the optimizer is attached to another model's encoder")
        if getattr(optimizer, "_graphed", None) is not None:
            raise RuntimeError("SharpnessAware: this optimizer's step is part of a captured GraphedTrainStep; a SAM step is two eager "
                               "passes and is not captured")
        self.model, self.optimizer = model, optimizer

    def step(self, **batch) -> Dict[str, torch.Tensor]:
        """One training step on ``batch`` (the keyword arguments of ``model.forward``, labels included): forward and backward,
        ``optimizer.perturb()``, forward and backward at the perturbed weights, ``optimizer.step()``, ``optimizer.zero_grad()``.
        Every pass computes the visual prompt and draws its dropout masks anew.  -> ``loss`` (first pass, detached), ``sam_loss``
        (second pass, detached), ``logits`` (first pass), ``grad_norm`` (0-dim device tensor: the first pass's global gradient
        norm, a copy of ``optimizer.last_sam_norm``).  If the second pass raises, the weights are put back before the exception
        leaves."""
        opt = self.optimizer
        first = self.model(**batch)
        if first.loss is None:
            raise ValueError("SharpnessAware.step needs a batch with labels: the first pass returned no loss")
        first.loss.backward()
        opt.perturb()
        try:
            second = self.model(**batch).loss
            second.backward()
        except BaseException:
            opt.unperturb()
            opt.zero_grad()
            raise
        opt.step()
        opt.zero_grad()
        return {"loss": first.loss.detach(), "sam_loss": second.detach(), "logits": first.logits,
                "grad_norm": opt.last_sam_norm.clone()}


def from_args(model: torch.nn.Module, args, optimizer):
    """-> the ``SharpnessAware`` that ``args`` asks for, or None at the default ``args.sam_rho = 0``."""
    if float(getattr(args, "sam_rho", 0.0) or 0.0) <= 0.0:
        return None
    return SharpnessAware(model, optimizer)
