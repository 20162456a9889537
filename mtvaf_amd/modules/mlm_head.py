"""Masked-LM head: BertOnlyMLMHead / RobertaLMHead with the loss at vocabulary width on the gfx950 kernels of csrc/mlm.hip
(DESIGN.md section 4.32).  Unlike the reference's heads it never forms the logits of every position: it gathers the selected rows,
runs the transform on them and hands them to ``engine.VocabCEFunction``, which sees the vocabulary one chunk at a time."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import engine


def _cfg(config, name, default=None):
    return config.get(name, default) if isinstance(config, dict) else getattr(config, name, default)


class _Transform(nn.Module):
    """reference: models/modeling_bert.py, BertPredictionHeadTransform"""

    def __init__(self, hidden: int, eps: float):
        super().__init__()
        self.dense = nn.Linear(hidden, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)


class _Predictions(nn.Module):
    """reference: models/modeling_bert.py, BertLMPredictionHead (decoder.bias IS bias, as there)"""

    def __init__(self, hidden: int, vocab: int, eps: float):
        super().__init__()
        self.transform = _Transform(hidden, eps)
        self.decoder = nn.Linear(hidden, vocab, bias=False)
        self.bias = nn.Parameter(torch.zeros(vocab))
        self.decoder.bias = self.bias


class MaskedLMHead(nn.Module):
    """``style="bert"``: parameters ``predictions.transform.dense``, ``predictions.transform.LayerNorm``, ``predictions.decoder``,
    ``predictions.bias`` (a checkpoint's ``cls.*``); ``style="roberta"``: ``dense``, ``layer_norm``, ``decoder``, ``bias``
    (``lm_head.*``).  ``word_embeddings`` (an ``nn.Embedding``): with ``tie`` the decoder's weight IS its table -- one Parameter,
    which then collects the embedding's and the decoder's gradient.  ``chunk``: logits columns alive at a time (None: the engine's
    default)."""

    def __init__(self, config, word_embeddings: Optional[nn.Embedding] = None, style: str = "bert", tie: bool = True,
                 chunk: Optional[int] = None):
        super().__init__()
        if style not in ("bert", "roberta"):
            raise ValueError(f"MaskedLMHead: style={style!r} (expected 'bert' or 'roberta')")
        H, V = _cfg(config, "hidden_size"), _cfg(config, "vocab_size")
        eps = _cfg(config, "layer_norm_eps", 1e-12)
        act = _cfg(config, "hidden_act", "gelu")
        if act != "gelu":
            raise NotImplementedError(f"MaskedLMHead: hidden_act={act!r}: only the exact (erf) GELU is on the kernel path")
        self.style, self.eps, self.chunk = style, float(eps), chunk
        if style == "bert":
            self.predictions = _Predictions(H, V, eps)
        else:
            self.dense = nn.Linear(H, H)
            self.layer_norm = nn.LayerNorm(H, eps=eps)
            self.decoder = nn.Linear(H, V, bias=False)
            self.bias = nn.Parameter(torch.zeros(V))
            self.decoder.bias = self.bias
        std = _cfg(config, "initializer_range", 0.02)
        self._dense().weight.data.normal_(mean=0.0, std=std)
        self._dense().bias.data.zero_()
        self._decoder().weight.data.normal_(mean=0.0, std=std)
        self.tied = bool(tie and word_embeddings is not None)
        if self.tied:
            if tuple(word_embeddings.weight.shape) != (V, H):
                raise ValueError(f"MaskedLMHead: word table {tuple(word_embeddings.weight.shape)} does not fit [{V}, {H}]")
            self._decoder().weight = word_embeddings.weight
        # 0-dim device tensors after a forward; never read here
        self.last_accuracy = self.last_count = self.last_stats = None

    def _dense(self):
        return self.predictions.transform.dense if self.style == "bert" else self.dense

    def _norm(self):
        return self.predictions.transform.LayerNorm if self.style == "bert" else self.layer_norm

    def _decoder(self):
        return self.predictions.decoder if self.style == "bert" else self.decoder

    def _bias(self):
        return self.predictions.bias if self.style == "bert" else self.bias

    def transform(self, hidden, positions):
        """The selected rows through dense + GELU + LayerNorm: [len(positions), H]."""
        x = engine.GatherRowsFunction.apply(hidden, positions)
        d, n = self._dense(), self._norm()
        x = engine.DenseGeluFunction.apply(x, d.weight, d.bias)
        return engine.RowLayerNormFunction.apply(x, n.weight, n.bias, self.eps)

    def logits(self, hidden, positions):
        """[len(positions), V] logits of the selected rows (dead slots: the logits of a zero row) -- on request only: this is the
        buffer the loss path never forms."""
        return engine.LinearFunction.apply(self.transform(hidden, positions), self._decoder().weight, self._bias(), False)

    def forward(self, hidden, positions, labels, count, reduction: str = "mean", return_logits: bool = False):
        """``hidden`` [B,S,H]; ``positions`` [cap] int32, ``labels`` [cap] int64, ``count`` [1] int32 as `mlm.mask_tokens` leaves
        them.  -> the loss (0-dim; "none": [cap] per-row losses, 0 in the dead slots); with ``return_logits`` (loss, logits
        [cap, V]) -- the logits are one more product on the transform output the loss read."""
        x = self.transform(hidden, positions)
        loss, rows, _lse, stats = engine.VocabCEFunction.apply(x, self._decoder().weight, self._bias(), labels, count, reduction,
                                                               self.chunk)
        live = stats[0]
        self.last_stats, self.last_count = stats, live
        self.last_accuracy = stats[1].float() / live.clamp(min=1).float()
        out = rows if reduction == "none" else loss
        if return_logits:
            return out, engine.LinearFunction.apply(x, self._decoder().weight, self._bias(), False)
        return out
