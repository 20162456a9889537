"""Host-side inputs of the candidate-span proposal (`TVNetSAModel.propose_spans` / `hip.span_propose`): the token -> word map
and the per-token word-string ids, built once per dataset from what the reference's features already hold.  Pure Python +
torch on the host; nothing here touches the GPU."""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence

import torch


def token_to_word(token_to_orig_map: Mapping[int, int], seq_len: int) -> torch.Tensor:
    """One feature's ``token_to_orig_map`` (token position -> index of its original word; the reference's
    models/utils.py:269-279) as an int32 ``[seq_len]`` row: -1 at every position outside the map ([CLS], [SEP], padding)."""
    row = torch.full((seq_len,), -1, dtype=torch.int32)
    for t, w in token_to_orig_map.items():
        if not 0 <= int(t) < seq_len or int(w) < 0:
            raise ValueError(f"token_to_orig_map entry {t}: {w} outside a sequence of {seq_len} tokens")
        row[int(t)] = int(w)
    return row


def batch_token_to_word(maps: Sequence[Mapping[int, int]], seq_len: int) -> torch.Tensor:
    """``[B, seq_len]`` int32 from the ``token_to_orig_map`` of every feature of a batch."""
    return torch.stack([token_to_word(m, seq_len) for m in maps])


def word_starts_from_labels(labels: torch.Tensor, x_id: int, attention_mask: torch.Tensor) -> torch.Tensor:
    """A synthetic ``token_to_word`` [B,S] int32 for callers who hold only ``X``-labelled features (`mtvaf_amd.words`): a token
    continues the previous word iff its label is ``x_id``.  Every other unmasked token -- [CLS] and [SEP] too -- starts a word,
    numbered from 0 along the sentence; masked tokens get -1.  The columns it gives are those of the tokenizer's map whenever the
    continuation pieces are exactly the ``X``-labelled ones (the word numbers differ: [CLS] counts as word 0 here)."""
    if tuple(labels.shape) != tuple(attention_mask.shape) or labels.dim() != 2:
        raise ValueError(f"labels {tuple(labels.shape)} and attention_mask {tuple(attention_mask.shape)}: expected two [B, S] tensors")
    live = torch.cumprod((attention_mask != 0).to(torch.int64), dim=1) != 0  # the leading ones
    starts = live & (labels != x_id)
    starts[:, 0] = live[:, 0]  # the first token opens a word whatever its label
    word = torch.cumsum(starts.to(torch.int64), dim=1) - 1
    return torch.where(live, word, torch.full_like(word, -1)).to(torch.int32)


def word_keys(sentences: Sequence[Sequence[str]], vocab: Optional[Dict[str, int]] = None):
    """Ids of the lower-cased word strings: equal strings (across sentences too) get equal ids, numbered from 0 in order of first
    appearance.  -> (one list of ids per sentence, the string -> id dict; pass it back in to keep numbering a further batch)."""
    vocab = {} if vocab is None else vocab
    ids = [[vocab.setdefault(w.lower(), len(vocab)) for w in words] for words in sentences]
    return ids, vocab


def token_word_keys(token_to_word_rows: torch.Tensor, word_ids: Sequence[Sequence[int]]) -> torch.Tensor:
    """Per-token key tensor ``[B, S]`` int32 for `span_propose`: the id (`word_keys`) of the word each in-map token belongs to,
    -1 outside the map."""
    out = torch.full_like(token_to_word_rows, -1)
    for b, ids in enumerate(word_ids):
        row = token_to_word_rows[b]
        m = row >= 0
        if bool(m.any()):
            out[b, m] = torch.tensor(ids, dtype=torch.int32)[row[m].long()]
    return out
