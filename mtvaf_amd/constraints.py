"""Per-position tag sets for the constrained CRF entry points (`CRF.partial_llh`, `CRF.constrained_marginals`,
`CRF.decode_constrained`; csrc/crf_lattice.hip), built on the device of their inputs with no host sync.

A set is one int64 word per column, read by the kernels as an unsigned 64-bit word: bit ``j`` set = tag ``j`` may be taken there.
A word without any of the low ``num_tags`` bits means "no constraint" (the full set), and bits at or above ``num_tags`` are
ignored, so 0 is the word of an unlabelled column.  With 64 tags bit 63 is the sign bit of the int64."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

MAX_TAGS = 64


def tag_word(tags: Iterable[int]) -> int:
    """The int64 value of the set word with the bits ``tags`` (each in 0..63) set; bit 63 makes it negative."""
    w = 0
    for j in tags:
        if not 0 <= int(j) < MAX_TAGS:
            raise ValueError(f"tag {j} outside 0..{MAX_TAGS - 1}")
        w |= 1 << int(j)
    return w - (1 << 64) if w >> 63 else w


def full_word(num_tags: int) -> int:
    """The word of the full set over ``num_tags`` tags."""
    if not 1 <= num_tags <= MAX_TAGS:
        raise ValueError(f"num_tags={num_tags} outside 1..{MAX_TAGS}")
    return tag_word(range(num_tags))


def sets_from_labels(labels: torch.Tensor, num_tags: int, unknown: Iterable[int] = ()) -> torch.Tensor:
    """labels [B,S] (any integer dtype) -> int64 [B,S]: the singleton ``{label}`` at a labelled column, and 0 (no constraint)
    where the label id is in ``unknown`` or outside ``[0, num_tags)`` -- e.g. the -100 / -1 of an unannotated token.  A fully
    labelled batch makes `CRF.partial_llh` the log-likelihood of `CRF.forward`; an unlabelled sentence costs exactly nothing."""
    if not 1 <= num_tags <= MAX_TAGS:
        raise ValueError(f"num_tags={num_tags} outside 1..{MAX_TAGS}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must hold integer ids, got {labels.dtype}")
    skip = {int(u) for u in unknown}
    table = torch.tensor([0 if j in skip else tag_word((j,)) for j in range(num_tags)] + [0], dtype=torch.int64,
                         device=labels.device)
    lab = labels.long()
    return table[torch.where((lab >= 0) & (lab < num_tags), lab, torch.full_like(lab, num_tags))]


def structural_sets(label_map: Dict[str, int], attention_mask: torch.Tensor, word_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What the layout of a tokenised sentence says about its tags -> int64 [B,S] set words.

    ``attention_mask`` [B,S] is a prefix mask; ``word_mask`` [B,S] (optional) marks the columns that carry a word (e.g. first
    sub-tokens).  Column 0 -> ``{[CLS]}``, the last unmasked column -> ``{[SEP]}``, the columns between them outside ``word_mask``
    -> ``{X}``, the word columns -> every tag but the structural ones (`mtvaf_amd.metrics.structural_labels`: PAD, X, [CLS],
    [SEP] for the reference's list; PAD is id 0 whether the map names it or not).  The tag count is ``max id + 1``.  A label
    that the map lacks leaves its columns unconstrained (word 0), as are the masked columns; a sentence of one column is its
    ``[CLS]``."""
    from .metrics import structural_labels
    num_tags = max(label_map.values()) + 1
    if min(label_map.values()) < 0 or not 1 <= num_tags <= MAX_TAGS:
        raise ValueError(f"label ids must lie in 0..{MAX_TAGS - 1}")
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask {tuple(attention_mask.shape)}: expected [B, S]")
    if word_mask is not None and tuple(word_mask.shape) != tuple(attention_mask.shape):
        raise ValueError(f"word_mask {tuple(word_mask.shape)} does not fit attention_mask {tuple(attention_mask.shape)}")
    structural = {label_map.get(n, 0) if n == "PAD" else label_map[n] for n in structural_labels(label_map)}
    word = tag_word(j for j in range(num_tags) if j not in structural)

    def single(name):
        return tag_word((label_map[name],)) if name in label_map else 0

    dev = attention_mask.device
    B, S = attention_mask.shape
    on = torch.cumprod((attention_mask != 0).to(torch.int64), dim=1)  # the leading ones
    lens = on.sum(dim=1, keepdim=True)
    col = torch.arange(S, device=dev)[None, :]

    def const(v):
        return torch.full((B, S), v, dtype=torch.int64, device=dev)

    sets = const(word)
    if word_mask is not None:
        sets = torch.where(word_mask.to(dev) != 0, sets, const(single("X")))
    sets = torch.where(col == lens - 1, const(single("[SEP]")), sets)
    sets = torch.where(col == 0, const(single("[CLS]")), sets)
    return torch.where(on != 0, sets, const(0))
