"""Word-level tagging head: the word axis of a batch and the pooling of piece vectors onto it.

`TVNetSAModel2` tags word pieces by default: continuation pieces carry the pseudo-label ``X`` and the chain runs over them.  With
``args.word_pooling`` the head reads ONE vector per word instead -- its first piece, its last piece or the mean of its pieces -- and
the chain runs over words.  The word axis keeps the layout every CRF kernel assumes ([CLS] in column 0, a prefix mask, [SEP] the last
live column), so likelihood, decoding, constraints, marginals, risk, entropy, sampling and the scorers run on it unchanged.

    index = build_word_index(attention_mask, token_to_word)          # device, no host sync (csrc/wordpool.hip)
    y = WordPooling("mean")(last_hidden_state, index)                # [B, W, H]; autograd through engine.WordPoolFunction
    wl = word_labels(labels, index)                                  # piece-level labels -> [B, W] by the first piece
    pieces = tags_to_pieces(word_tags, index, fill=label_map["X"])   # and back, for a per-position evaluation

``token_to_word`` is the map of `mtvaf_amd.spans.batch_token_to_word` (int32, -1 outside the map);
`mtvaf_amd.spans.word_starts_from_labels` makes one from ``X``-labelled features.  The helpers below are plain torch (index
plumbing on whatever device the index lives on); the pooling itself has no torch fallback."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import nn

from . import engine, hip

MODES = ("first", "last", "mean")


class WordIndex(NamedTuple):
    """The outputs of `hip.word_index` (include/mtvaf_hip.h, mtvaf_word_index).  A token s below the sentence's length opens a
    column iff s == 0, map[s] < 0 or map[s] != map[s-1]."""
    col_start: torch.Tensor     # [B,W] int32: first token of the column (0 on dead columns)
    col_len: torch.Tensor       # [B,W] int32: its tokens, 0 = no column
    col_of_token: torch.Tensor  # [B,S] int32: -1 for masked tokens and for tokens of columns beyond W
    word_mask: torch.Tensor     # [B,W] uint8: live columns, a prefix mask
    word_id: torch.Tensor       # [B,W] int32: the column's map value, -1 for unmapped tokens and dead columns
    n_cols: torch.Tensor        # [B] int32: the true column count (it may exceed W: the columns beyond W are dropped)

    @property
    def width(self) -> int:
        return self.col_start.shape[1]


def build_word_index(attention_mask, token_to_word, max_words: Optional[int] = None) -> WordIndex:
    """attention_mask [B,S] (a prefix mask, on the device), token_to_word [B,S] (any integer dtype, any device) -> `WordIndex` of
    width ``max_words`` (default S, which always suffices: nothing is read back to size it).  One launch, no host sync."""
    if tuple(token_to_word.shape) != tuple(attention_mask.shape):
        raise ValueError(f"token_to_word {tuple(token_to_word.shape)} does not fit attention_mask {tuple(attention_mask.shape)}")
    t2w = token_to_word.to(device=attention_mask.device, dtype=torch.int32).contiguous()
    return WordIndex(**hip.word_index(attention_mask, t2w, max_words))


class WordPooling(nn.Module):
    """``forward(x [B,S,H], index) -> [B,W,H]``: the pieces of every word pooled (first | last | mean), zeros on dead columns."""

    def __init__(self, mode: str = "first"):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"WordPooling: mode {mode!r}: expected one of {MODES}")
        self.mode = mode

    def forward(self, x, index: WordIndex):
        return engine.WordPoolFunction.apply(x, index, self.mode)

    def extra_repr(self):
        return f"mode={self.mode!r}"


def _first_piece(values, index: WordIndex):
    """values [B,S] -> [B,W]: the value at every column's first piece, 0 on dead columns."""
    if values.dim() != 2 or values.shape[0] != index.col_start.shape[0] or values.shape[1] != index.col_of_token.shape[1]:
        raise ValueError(f"a [B,S] tensor of shape {tuple(values.shape)} does not fit an index over "
                         f"{tuple(index.col_of_token.shape)} tokens")
    start = index.col_start.to(values.device).long()
    live = index.word_mask.to(values.device) != 0
    return torch.where(live, values.gather(1, start), torch.zeros((), dtype=values.dtype, device=values.device))


def word_labels(labels, index: WordIndex):
    """Piece-level labels [B,S] -> word-level [B,W]: the label of the column's first piece, 0 on dead columns."""
    return _first_piece(labels, index)


def word_allowed(allowed, index: WordIndex):
    """Piece-level constraint words [B,S] (`mtvaf_amd.constraints`) -> [B,W] by the column's first piece, 0 (unconstrained) on dead
    columns."""
    return _first_piece(allowed, index)


def tags_to_pieces(word_tags, index: WordIndex, fill: int, pad: int = 0):
    """Word tags [B,W] back onto piece positions [B,S]: the word's tag on its first piece, ``fill`` (the ``X`` id) on its
    continuation pieces, ``pad`` on masked tokens and on tokens of columns beyond W -- the layout the reference trainer's
    per-position evaluation reads."""
    col = index.col_of_token.to(word_tags.device).long()
    if word_tags.dim() != 2 or tuple(word_tags.shape) != tuple(index.col_start.shape):
        raise ValueError(f"word_tags {tuple(word_tags.shape)} do not fit an index of {tuple(index.col_start.shape)} columns")
    safe = col.clamp_min(0)
    start = index.col_start.to(word_tags.device).long().gather(1, safe)
    pos = torch.arange(col.shape[1], device=word_tags.device)[None, :]
    const = lambda v: torch.full((), v, dtype=word_tags.dtype, device=word_tags.device)
    out = torch.where(start == pos, word_tags.gather(1, safe), const(fill))
    return torch.where(col >= 0, out, const(pad))
