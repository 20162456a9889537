"""Masked-LM data path on the device (csrc/mlm.hip): choosing and corrupting tokens by the rule of
Hugging Face's ``DataCollatorForLanguageModeling``, compacting the chosen rows, and gathering their hidden states.  Nothing here
reads a device value on the host: the number of chosen tokens stays a device word and every buffer has a fixed capacity."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import engine, hip


def default_capacity(tokens: int, probability: float) -> int:
    """Rows the head runs on for ``tokens`` = B * S positions: twice the expected selection, rounded up to 32, at most all."""
    return max(1, min(tokens, (math.ceil(2.0 * probability * tokens) + 31) // 32 * 32))


def _u8(mask: torch.Tensor) -> torch.Tensor:
    return (mask if mask.dtype == torch.uint8 else mask.ne(0).view(torch.uint8)).contiguous()


def mask_tokens(input_ids: torch.Tensor, attention_mask: torch.Tensor, *, mask_token_id: int, vocab_size: int,
                special_ids: Sequence[int], probability: float = 0.15, capacity: Optional[int] = None,
                special_mask: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None) -> dict:
    """``input_ids`` [B,S] integer ids and ``attention_mask`` [B,S] (non-zero = attended, any pattern) on the device.  A token that
    is attended, not marked in ``special_mask`` [B,S] and none of the (at most 8) ``special_ids`` is selected iff u0 <
    ``probability``; a selected token becomes ``mask_token_id`` if u1 < 0.8, else the id min(V - 1, int(u2 * V)) if u1 < 0.9, else
    stays.  ``uniforms`` [B,S,3] fp32 in [0, 1): drawn from the dropout generator (``engine.RNG``, one offset per call) unless
    handed in.  At most ``capacity`` tokens are selected, in row-major order; later ones stay as they are.
    -> dict: ``input_ids`` [B,S] (corrupted), ``positions`` [capacity] int32 (flat b * S + t ascending, -1 in the dead tail),
    ``labels`` [capacity] int64 (original ids, -100 in the dead tail), ``count`` [1] int32, ``stats`` [3] int32 (eligible,
    selected, dropped for capacity), ``uniforms``."""
    if input_ids.dim() != 2 or attention_mask.shape != input_ids.shape:
        raise ValueError(f"mask_tokens: input_ids {tuple(input_ids.shape)} and attention_mask {tuple(attention_mask.shape)} must be "
                         "[B, S] both")
    if not 0.0 <= probability <= 1.0:
        raise ValueError(f"mask_tokens: probability={probability!r} (expected a number in [0, 1])")
    if not 0 <= mask_token_id < vocab_size:
        raise ValueError(f"mask_tokens: mask_token_id={mask_token_id} outside the vocabulary of {vocab_size}")
    B, S = input_ids.shape
    if special_mask is not None and special_mask.shape != input_ids.shape:
        raise ValueError(f"mask_tokens: special_mask {tuple(special_mask.shape)} does not fit input_ids {tuple(input_ids.shape)}")
    if capacity is None:
        capacity = default_capacity(B * S, probability)
    ids = input_ids.long().contiguous()
    if uniforms is None:
        uniforms = torch.empty(B, S, 3, dtype=torch.float32, device=ids.device)
        hip.uniform_fill(uniforms, engine.RNG.seed(), engine.RNG.next())
    elif uniforms.shape != (B, S, 3):
        raise ValueError(f"mask_tokens: uniforms {tuple(uniforms.shape)} (expected {(B, S, 3)})")
    uniforms = uniforms.float().contiguous()
    ids_out, positions, labels, count, stats = hip.mlm_mask(ids, _u8(attention_mask), None if special_mask is None else
                                                            _u8(special_mask), uniforms, special_ids, probability, mask_token_id,
                                                            vocab_size, capacity)
    return {"input_ids": ids_out, "positions": positions, "labels": labels, "count": count, "stats": stats, "uniforms": uniforms}


def compact_labels(labels: torch.Tensor, vocab_size: int, capacity: Optional[int] = None):
    """Hugging Face's ``labels`` [B,S] (-100 = not predicted) -> (positions [capacity] int32, labels [capacity] int64, count [1]
    int32) by the masking kernel itself: the labels go in as the ids, "attended" is ``labels != -100`` and every such token is
    selected (probability 1), so positions / labels / count come out exactly as a masking call leaves them.  ``capacity``: B * S
    unless the caller knows a bound (tokens beyond it are dropped)."""
    if labels.dim() != 2:
        raise ValueError(f"compact_labels: labels {tuple(labels.shape)} must be [B, S]")
    B, S = labels.shape
    lab = labels.long().contiguous()
    zeros = torch.zeros(B, S, 3, dtype=torch.float32, device=lab.device)
    _, positions, out, count, _ = hip.mlm_mask(lab, lab.ne(-100).view(torch.uint8), None, zeros, (), 1.0, 0, vocab_size,
                                               B * S if capacity is None else capacity)
    return positions, out, count


def gather_rows(hidden: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
    """``hidden`` [B,S,H] (or [rows,H]) -> [len(positions), H]: the rows at the flat ``positions``, zero rows where a position is
    -1.  Differentiable in ``hidden``: each position's gradient row goes back to its place, zeros elsewhere."""
    return engine.GatherRowsFunction.apply(hidden, positions)
