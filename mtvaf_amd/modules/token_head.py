"""Softmax tagging head: token-level cross entropy with class weights, label smoothing and the focal factor, and per-token
decoding, on the gfx950 kernels mtvaf_token_ce_{fwd,bwd} / mtvaf_token_argmax (csrc/token_ce.hip).
The module holds no trainable parameter: the class weights are a buffer."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from .. import engine, hip


def zero_chain(num_tags: int):
    """A `CRF` whose start, end and transition scores are zero BUFFERS (no parameter, no state-dict key): under it the posterior
    over paths is the product of the token softmaxes, so `CRF.entities` reports sums of token log-probabilities and
    `CRF.marginals` the softmax -- the chain a softmax head hands to the code that expects one."""
    from .crf import CRF
    crf = CRF(num_tags, batch_first=True)
    for name in ("start_transitions", "end_transitions", "transitions"):
        shape = getattr(crf, name).shape
        delattr(crf, name)
        crf.register_buffer(name, torch.zeros(shape), persistent=False)
    return crf


class TokenCrossEntropy(nn.Module):
    REDUCTIONS = ("mean", "batch_mean", "sum", "none")

    def __init__(self, num_tags: int, class_weight: Optional[Sequence[float]] = None, smoothing: float = 0.0,
                 focal_gamma: float = 0.0, ignore_index: int = -100) -> None:
        super().__init__()
        if not 1 <= num_tags <= 64:
            raise ValueError(f"num_tags={num_tags}: the token kernels support 1..64 tags (one tag per lane of a wavefront)")
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing={smoothing!r}: expected a number in [0, 1)")
        if not (focal_gamma == 0.0 or 1.0 <= focal_gamma <= 8.0):
            raise ValueError(f"focal_gamma={focal_gamma!r}: expected 0 or a number in [1, 8]")
        self.num_tags, self.smoothing, self.focal_gamma, self.ignore_index = num_tags, float(smoothing), float(focal_gamma), int(ignore_index)
        weight = None
        if class_weight is not None:
            weight = torch.as_tensor(class_weight, dtype=torch.float32).detach().clone().view(-1)
            if weight.numel() != num_tags or not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError(f"class_weight: expected {num_tags} finite weights >= 0, got {class_weight!r}")
        self.register_buffer("class_weight", weight)
        self.last_stats = None  # int32 [2] on the device after a forward: live rows, out-of-range labels; never read here

    def extra_repr(self) -> str:
        return (f"num_tags={self.num_tags}, smoothing={self.smoothing}, focal_gamma={self.focal_gamma}, "
                f"ignore_index={self.ignore_index}, class_weight={'yes' if self.class_weight is not None else 'no'}")

    def _check(self, logits):
        if logits.dim() not in (2, 3) or logits.shape[-1] != self.num_tags:
            raise ValueError(f"expected logits [*, {self.num_tags}] or [*, *, {self.num_tags}], got {tuple(logits.shape)}")

    def forward(self, logits, labels, mask: Optional[torch.Tensor] = None, reduction: str = "mean", scale: float = 1.0):
        """``logits`` [B,S,C] or [N,C], ``labels`` and ``mask`` their leading shape.  "mean": the sum over the live tokens by the
        sum of their class weights -- at focal_gamma 0 ``torch.nn.functional.cross_entropy``; "batch_mean": by B, commensurable
        with the CRF's mean NLL; "sum"; all times ``scale``, inside the kernel -> 0-dim.  "none": every token's value in the shape
        of ``labels``, 0 on dead tokens, differentiable per token (``scale`` is not applied)."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        self._check(logits)
        loss, rows, stats = engine.TokenCEFunction.apply(logits, labels, mask, self.class_weight, self.ignore_index, self.smoothing,
                                                         self.focal_gamma, reduction, scale)
        self.last_stats = stats
        return rows.view(labels.shape) if reduction == "none" else loss

    @torch.no_grad()
    def decode(self, logits, mask: Optional[torch.Tensor] = None, allowed: Optional[torch.Tensor] = None):
        """-> (tags int64, logp fp32), both in the leading shape of ``logits``: every live token's first maximum and its
        log-probability; 0 and 0 on masked tokens.  ``allowed``: int64 tag sets (`mtvaf_amd.constraints`; 0 = no constraint) --
        the maximum then runs over the permitted tags, ``logp`` stays the unconstrained log-probability.  No host sync."""
        self._check(logits)
        lead = logits.shape[:-1]
        zc = logits.detach().contiguous().float().view(-1, self.num_tags)
        N = zc.shape[0]
        if (mask is not None and mask.numel() != N) or (allowed is not None and allowed.numel() != N):
            raise ValueError(f"mask / allowed do not fit logits {tuple(logits.shape)}")
        m8 = None if mask is None else mask.ne(0).contiguous().view(torch.uint8).view(-1)
        sets = None if allowed is None else allowed.to(zc.device).contiguous().view(-1).long()
        tags = torch.empty(N, dtype=torch.int64, device=zc.device)
        logp = torch.empty(N, dtype=torch.float32, device=zc.device)
        hip.token_argmax(zc, m8, sets, tags, logp)
        return tags.view(lead), logp.view(lead)
