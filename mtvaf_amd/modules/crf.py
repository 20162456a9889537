"""Linear-chain CRF module with the public surface of ``torchcrf.CRF`` as the reference uses it
(models/bert_model.py:464 ``CRF(num_labels, batch_first=True)``, :511 ``decode``, :521
``crf(emissions, labels, mask=..., reduction='mean')``), computed by the gfx950 kernels
mtvaf_crf_nll_{fwd,bwd} / mtvaf_crf_llh_{fwd,bwd} / mtvaf_crf_marginals / mtvaf_crf_viterbi / mtvaf_crf_nbest / mtvaf_crf_sample
(``sample``, and ``minimum_risk`` over a sampled hypothesis set), and over per-position
tag sets by mtvaf_crf_lattice_{fwd,bwd,marginals,viterbi} (``partial_llh``, ``constrained_marginals``, ``decode_constrained``), and
the gradient of posterior expectations by mtvaf_crf_risk_{fwd,bwd} (``expected_cost``, ``hamming_risk``, ``differentiable_marginals``)
and, with edge costs, mtvaf_crf_path_{fwd,bwd} (``expected_path_cost``, ``entropy``, ``kl_divergence``).  Parameter names (``start_transitions``,
``end_transitions``, ``transitions``) and the uniform(-0.1, 0.1) initialisation follow pytorch-crf.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
from torch import nn

from .. import engine, hip


class DeferredTags(list):
    """``List[List[int]]`` of Viterbi paths whose device->host copy has been ENQUEUED but not waited for.

    The reference's ``crf.decode`` returns Python lists, which forces a host sync in the middle of every training
    step (models/bert_model.py:511).  This list subclass carries the packed
    [B, S+1] int32 result (tags | length) in pinned host memory plus the copy's event and fills itself on first
    use (indexing, iteration, len, comparison, repr ...), i.e. where the trainer builds y_pred after
    ``loss.backward()`` (modules/train.py:627-647).  Values are identical to an eager ``decode``."""

    def __init__(self, packed_host: torch.Tensor, event, S: int, release=None):
        super().__init__()
        self._packed, self._event, self._S, self._release = packed_host, event, S, release
        self.device_tags = None  # decode_deferred: the [B, S] int32 device tensor of the same Viterbi launch (-1 beyond each length)

    def _fill(self):
        if self._packed is not None:
            if self._event is not None:
                self._event.synchronize()
            packed, S = self._packed, self._S
            self._packed = None
            rows, lens = packed[:, :S].tolist(), packed[:, S].tolist()
            super().extend(row[:n] for row, n in zip(rows, lens))
            self._give_back()
        return self

    def packed(self):
        """The packed [B, S+1] int32 host array (tags padded with -1 | length) after waiting for the copy, or None once
        the list has been materialised -- array consumers (``mtvaf_amd.metrics.label_sequences``) skip the Python lists."""
        if self._packed is None:
            return None
        if self._event is not None:
            self._event.synchronize()
        return self._packed.numpy()

    def _give_back(self):
        if self._release is not None:
            self._release()
            self._release = None

    def __del__(self):  # never read: the staging buffer goes back with its (possibly pending) copy event
        self._give_back()

    def __getitem__(self, i):
        self._fill()
        return super().__getitem__(i)

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __len__(self):
        self._fill()
        return super().__len__()

    def __eq__(self, other):
        self._fill()
        return list(self) == (list(other) if isinstance(other, list) else other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def __repr__(self):
        self._fill()
        return super().__repr__()

    def __reduce__(self):
        return (list, (list(self),))


class CRF(nn.Module):
    def __init__(self, num_tags: int, batch_first: bool = False) -> None:
        if num_tags <= 0:
            raise ValueError(f"invalid number of tags: {num_tags}")
        if num_tags > 64:
            raise NotImplementedError(f"num_tags={num_tags}: the CRF kernels support at most 64 tags (one tag per lane "
                                      f"of a wavefront)")
        super().__init__()
        self.num_tags = num_tags
        self.batch_first = batch_first
        self.start_transitions = nn.Parameter(torch.empty(num_tags))
        self.end_transitions = nn.Parameter(torch.empty(num_tags))
        self.transitions = nn.Parameter(torch.empty(num_tags, num_tags))
        # pinned staging buffers of decode_deferred, recycled: a fresh pinned allocation per step costs a
        # hipHostMalloc that waits for the GPU to drain (measured 185 ms per step at B=128, S=512)
        self._host_pool: list = []
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.uniform_(self.start_transitions, -0.1, 0.1)
        nn.init.uniform_(self.end_transitions, -0.1, 0.1)
        nn.init.uniform_(self.transitions, -0.1, 0.1)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(num_tags={self.num_tags})"

    def _prep(self, emissions, tags, mask):
        if emissions.dim() != 3 or emissions.size(2) != self.num_tags:
            raise ValueError(f"expected emissions [*, *, {self.num_tags}], got {tuple(emissions.shape)}")
        if not self.batch_first:
            emissions = emissions.transpose(0, 1)
            tags = tags.transpose(0, 1) if tags is not None else None
            mask = mask.transpose(0, 1) if mask is not None else None
        B, S, _ = emissions.shape
        if mask is None:
            mask = torch.ones(B, S, dtype=torch.uint8, device=emissions.device)
        mask = mask.to(torch.uint8).contiguous()
        if tags is not None:
            tags = tags.to(torch.long).contiguous()
        return emissions.float(), tags, mask

    REDUCTIONS = ("none", "sum", "mean", "token_mean")

    def forward(self, emissions, tags, mask: Optional[torch.Tensor] = None, reduction: str = "sum"):
        """Log-likelihood of ``tags`` with torchcrf's reductions.  'mean' and 'sum' come from the fused batch-mean NLL
        kernels ('sum' is mean * B).  'none' returns the per-sentence log-likelihoods [B] from mtvaf_crf_llh_{fwd,bwd},
        whose backward takes a per-sentence upstream gradient, so ``(w * crf(..., reduction='none')).sum()`` weights
        sentences inside the kernels; 'token_mean' is ``llh.sum() / mask.sum()`` on top of it.  Any other string raises
        ValueError."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        emissions, tags, mask = self._prep(emissions, tags, mask)
        if reduction in ("none", "token_mean"):
            llh = engine.CRFLLHFunction.apply(emissions, self.start_transitions, self.end_transitions, self.transitions,
                                              tags, mask)
            if reduction == "none":
                return llh
            return llh.sum() / mask.to(llh.dtype).sum()
        nll_mean = engine.CRFNLLFunction.apply(emissions, self.start_transitions, self.end_transitions,
                                               self.transitions, tags, mask)
        if reduction == "mean":
            return -nll_mean
        return -nll_mean * emissions.shape[0]

    @torch.no_grad()
    def marginals(self, emissions, mask: Optional[torch.Tensor] = None, return_logz: bool = False):
        """Posterior tag probabilities ``p(y_t = j | emissions)``: [B,S,C] (``batch_first``) or [S,B,C], exact zeros at
        masked steps; with ``return_logz`` also the log-partition ``logZ`` [B].  Computed by mtvaf_crf_marginals (the
        forward / backward recursions without gold path, edge marginals or parameter gradients).  Runs under
        ``torch.no_grad()``: the result does not require grad and no gradient flows through it."""
        emissions, _, mask = self._prep(emissions, None, mask)
        B, S, C = emissions.shape
        em = emissions.contiguous()
        ws, wsb = hip.crf_workspace(B, S, C, em.device)
        marg = torch.empty_like(em)
        logz = torch.empty(B, dtype=em.dtype, device=em.device) if return_logz else None
        hip.crf_marginals(em, mask, self.start_transitions.data, self.end_transitions.data, self.transitions.data, marg,
                          logz, ws, wsb)
        if not self.batch_first:
            marg = marg.transpose(0, 1)
        return (marg, logz) if return_logz else marg

    def nll_mean(self, emissions, tags, mask: Optional[torch.Tensor] = None):
        """``-1 * self(emissions, tags, mask=mask, reduction='mean')`` (models/bert_model.py:521) as ONE autograd node: the
        kernel's result is that quantity, so the two negations (and their two backward kernels) are not launched."""
        emissions, tags, mask = self._prep(emissions, tags, mask)
        return engine.CRFNLLFunction.apply(emissions, self.start_transitions, self.end_transitions, self.transitions,
                                           tags, mask)

    @torch.no_grad()
    def decode_packed(self, emissions, mask: Optional[torch.Tensor] = None):
        """Viterbi on device -> (tags int32 [B,S] padded with -1, lengths int32 [B]); no host sync."""
        emissions, _, mask = self._prep(emissions, None, mask)
        B, S, _ = emissions.shape
        em = emissions.contiguous()
        tags = torch.empty(B, S, dtype=torch.int32, device=em.device)
        lens = torch.empty(B, dtype=torch.int32, device=em.device)
        hip.crf_viterbi(em, mask, self.start_transitions.data, self.end_transitions.data, self.transitions.data, tags,
                        lens)
        return tags, lens

    @torch.no_grad()
    def decode_nbest(self, emissions, mask: Optional[torch.Tensor] = None, nbest: int = 4, return_logprob: bool = True) -> dict:
        """The ``nbest`` (1..8) best tag sequences of every sentence on the device (mtvaf_crf_nbest); no host sync, nothing copied.

        ``mask`` is a prefix mask (ones, then zeros); emissions and mask follow ``batch_first``, every result is batch-first.
        -> dict: tags [B,K,S] int32 (row k the k-th best path, -1 behind the sentence), scores [B,K] (unnormalised path scores,
        non-increasing), logprob [B,K] = score - logZ (None without ``return_logprob``), n_paths [B] int32 = min(K, C^length):
        ranks >= n_paths hold tags -1, score -inf and logprob -inf.  Equal scores: the lower previous tag first, then the lower
        previous rank, so row 0 is ``decode_packed``'s path.  `mtvaf_amd.metrics.nbest_to_lists` turns it into Python lists."""
        emissions, _, mask = self._prep(emissions, None, mask)
        tags, scores, logprob, n_paths = hip.crf_nbest(emissions.contiguous(), mask, self.start_transitions.data,
                                                       self.end_transitions.data, self.transitions.data, nbest, return_logprob)
        return {"tags": tags, "scores": scores, "logprob": logprob, "n_paths": n_paths}

    @torch.no_grad()
    def sample(self, emissions, mask: Optional[torch.Tensor] = None, n_samples: int = 8, uniforms: Optional[torch.Tensor] = None,
               return_logprob: bool = True, return_uniforms: bool = False) -> dict:
        """``n_samples`` (1..64) tag sequences of every sentence drawn from the posterior ``p(y | emissions)`` on the device
        (mtvaf_crf_sample: forward-filter backward-sample); no host sync.

        ``mask`` is a prefix mask; emissions and mask follow ``batch_first``, every result is batch-first.  Without ``uniforms``
        the draws come from the dropout generator: seed ``engine.RNG.seed()`` and ONE offset ``engine.RNG.next(1)`` per call, as a
        dropout site takes.  ``uniforms`` float32 [B,K,S] in [0,1) (batch-first) supplies the uniform of every draw instead and
        leaves ``engine.RNG`` alone: the call is then a pure function of its arguments.
        -> dict: tags [B,K,S] int32 (-1 behind the sentence), scores [B,K] (unnormalised path scores), logprob [B,K] = score -
        logZ (None without ``return_logprob``) and, with ``return_uniforms``, uniforms [B,K,S] (those used; 0 behind the
        sentence).  Nothing here carries a gradient: a differentiable log-probability of a sample is
        ``self(emissions, tags, mask, reduction="none")`` on its tags, and ``minimum_risk`` builds a loss on a sampled set."""
        emissions, _, mask = self._prep(emissions, None, mask)
        if uniforms is None:
            seed, offset = engine.RNG.seed(), engine.RNG.next(1)
        else:
            seed, offset, uniforms = 0, 0, uniforms.float().contiguous()
        tags, scores, logprob, uout = hip.crf_sample(emissions.contiguous(), mask, self.start_transitions.data,
                                                     self.end_transitions.data, self.transitions.data, n_samples, uniforms, seed,
                                                     offset, return_logprob, return_uniforms)
        out = {"tags": tags, "scores": scores, "logprob": logprob}
        if return_uniforms:
            out["uniforms"] = uout
        return out

    def minimum_risk(self, emissions, hypotheses, cost, mask: Optional[torch.Tensor] = None, alpha: float = 1.0,
                     reduction: str = "none"):
        """Minimum-risk training over a hypothesis set: ``risk[b] = sum_k q_k cost[b,k]`` with ``q = softmax_k(alpha * llh_k)``, the
        posterior renormalised over the set, for a cost of whole tag sequences that need not decompose (sentence F1:
        `mtvaf_amd.metrics.sentence_f1_cost`).

        ``hypotheses`` int [B,K,S] batch-first (``sample``'s / ``decode_nbest``'s tags, rows may be concatenated); a row is valid
        iff its first column is >= 0, and a row identical to an earlier valid row of the same sentence (over the unmasked columns)
        is dropped.  ``cost`` [B,K] carries no gradient.  ``llh_k`` comes from mtvaf_crf_llh_{fwd,bwd} at B * K rows, so the
        gradient flows to the emissions and to the chain parameters.  A sentence without a valid row has risk 0 and no gradient.
        Reductions as ``forward``: 'none' [B], 'sum', 'mean' (over sentences), 'token_mean' (sum / mask.sum())."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        em, _, mask = self._prep(emissions, None, mask)
        B, S, C = em.shape
        if hypotheses.dim() != 3 or hypotheses.shape[0] != B or hypotheses.shape[2] != S or hypotheses.dtype.is_floating_point:
            raise ValueError(f"CRF.minimum_risk: hypotheses {tuple(hypotheses.shape)} {hypotheses.dtype}: expected int [{B}, K, {S}]")
        K = hypotheses.shape[1]
        if tuple(cost.shape) != (B, K):
            raise ValueError(f"CRF.minimum_risk: cost {tuple(cost.shape)} does not fit hypotheses [{B}, {K}, {S}]")
        on = (mask != 0)[:, None, :]
        hyp = torch.where(on, hypotheses.long(), torch.full((), -1, dtype=torch.long, device=em.device))
        valid = hypotheses[:, :, 0] >= 0
        same = (hyp[:, :, None, :] == hyp[:, None, :, :]).all(-1) & valid[:, None, :]      # [b,k,k']: k' valid and equal to k
        valid = valid & ~torch.tril(same, diagonal=-1).any(-1)                              # no earlier valid twin
        llh = engine.CRFLLHFunction.apply(em[:, None].expand(B, K, S, C).reshape(B * K, S, C), self.start_transitions,
                                          self.end_transitions, self.transitions, hyp.clamp(0, C - 1).reshape(B * K, S),
                                          mask[:, None].expand(B, K, S).reshape(B * K, S).contiguous()).view(B, K)
        z = torch.where(valid, alpha * llh, torch.full((), float("-inf"), device=em.device))
        top = z.detach().max(dim=1, keepdim=True).values
        e = torch.exp(z - torch.where(torch.isfinite(top), top, torch.zeros_like(top)))    # 0 at dropped rows
        den = e.sum(dim=1, keepdim=True)                                                    # >= 1 with a valid row, else 0
        q = e / torch.where(den > 0, den, torch.ones_like(den))
        risk = (q * cost.detach().to(q.dtype)).sum(dim=1)
        return self.reduce_risk(risk, mask.to(risk.dtype).sum(), reduction)

    @torch.no_grad()
    def entities(self, emissions, mask, tables, tags=None, keep=None, max_entities: int = 32) -> dict:
        """The entities of decoded tags with the posterior of each decoded segment (mtvaf_crf_entities); no host sync.

        ``mask`` is a prefix mask (ones, then zeros); ``tables`` the dict of ``mtvaf_amd.metrics.entity_tables`` or the device
        tensors ``entity_device_tables`` made of it; ``tags`` [B,>=S] int32 as ``decode_packed`` returns them (None: decoded
        here); ``keep`` [B,S] the columns that take part in chunking (None: columns 1 .. L-1).  ``tags``, ``keep`` and every
        result are batch-first; emissions and mask follow ``batch_first`` as everywhere else.
        -> dict: tags [B,S] int32, lengths [B] int32, entities [B,E,3] int32 (start column, end column, type index; -1 in
        unused slots), log_confidence [B,E] = log p(y_b..y_e = decoded tags | x), confidence [B,E] = its exp (0 in unused
        slots), count [B] int32 (may exceed E = max_entities: the first E chunks by end column are stored)."""
        from ..metrics import entity_device_tables
        emissions, _, mask = self._prep(emissions, None, mask)
        B, S, C = emissions.shape
        em = emissions.contiguous()
        t = entity_device_tables(tables, em.device)
        if tags is None:  # (decode_packed on the prepared tensors)
            tags = torch.empty(B, S, dtype=torch.int32, device=em.device)
            lengths = torch.empty(B, dtype=torch.int32, device=em.device)
            hip.crf_viterbi(em, mask, self.start_transitions.data, self.end_transitions.data, self.transitions.data, tags,
                            lengths)
        else:
            lengths = mask.sum(dim=1, dtype=torch.int32)
            if tags.dtype != torch.int32:
                tags = tags.to(torch.int32)
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        ents, log_conf, count = hip.crf_entities(em, mask, tags, keep, self.start_transitions.data, self.end_transitions.data,
                                                 self.transitions.data, t["start"], t["end"], t["type_of"], t["n_types"],
                                                 max_entities)
        conf = torch.where(ents[..., 0] >= 0, torch.exp(log_conf), torch.zeros_like(log_conf))
        return {"tags": tags[:, :S], "lengths": lengths, "entities": ents, "log_confidence": log_conf, "confidence": conf,
                "count": count}

    @torch.no_grad()
    def chunk_posteriors(self, emissions, mask, tables, keep=None, allowed=None, max_width: int = 8, check: bool = False):
        """The posterior of every chunk EVENT (mtvaf_crf_chunk_posteriors): for every span of kept columns and every type, the
        probability that the chunker of ``entities`` emits exactly that chunk -- a start at its first column, no start after
        it, an end at its last column, that type -- under the chain restricted to the tag sets ``allowed``.  No host sync.

        ``mask`` / ``tables`` / ``keep`` as for ``entities`` (``keep`` None: columns 1 .. L-1); ``allowed`` int64 [B,S] set words
        as for ``partial_llh`` (None: no constraint) -- the posteriors are conditional on them.  ``keep`` and ``allowed`` are
        batch-first like every result.  A non-kept column strictly between two kept columns must carry a singleton set (the X of
        a sub-word piece under `mtvaf_amd.constraints.structural_sets`); where it does not, the kernel takes the lowest tag of
        its set, which is outside the contract -- ``check=True`` verifies it on the host (one sync) and raises ValueError.
        -> (log_post [B,S,max_width,n_types], logz_a [B]): ``log_post[s, b, w, T]`` for the span of ``w + 1`` kept columns that
        starts at column ``b``; -inf where the event is impossible or undefined (``b`` not kept or behind the sentence, the span
        past the last kept column).  ``max_width`` 1..16.  Ends strictly inside a span do not exclude it, as in the chunker."""
        from ..metrics import entity_device_tables
        emissions, _, mask = self._prep(emissions, None, mask)
        B, S, C = emissions.shape
        em = emissions.contiguous()
        t = entity_device_tables(tables, em.device)
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        if allowed is not None:
            hip.crf_lattice_check(em, allowed, mask, "CRF.chunk_posteriors")
            allowed = allowed.contiguous()
        if check:
            on = torch.cumprod(mask.long(), dim=1).bool()
            kp = (keep.bool() if keep is not None else torch.arange(S, device=em.device)[None, :] >= 1) & on
            inner = ~kp & on & (torch.cumsum(kp.long(), dim=1) > 0) & (torch.flip(torch.cumsum(torch.flip(kp.long(), [1]), 1), [1]) > 0)
            bits = torch.ones(B, S, C, dtype=torch.bool, device=em.device) if allowed is None else \
                ((allowed[..., None] >> torch.arange(C, device=em.device)) & 1).bool()
            size = bits.sum(-1)
            size = torch.where(size == 0, torch.full_like(size, C), size)
            if bool((inner & (size != 1)).any()):
                raise ValueError("CRF.chunk_posteriors: a non-kept column between two kept columns carries a set of more than one tag")
        return hip.crf_chunk_posteriors(em, allowed, mask, keep, self.start_transitions.data, self.end_transitions.data,
                                        self.transitions.data, t["start"], t["end"], t["type_of"], t["n_types"], max_width)

    @staticmethod
    def entity_chunk_confidence(ents, log_post, keep):
        """The chunk-event log posterior of given entities, gathered from ``chunk_posteriors``' ``log_post`` [B,S,W,n_types]:
        ``ents`` [B,E,3] as ``entities`` returns them (start column, end column, type; -1 in unused slots), ``keep`` [B,S] the
        kept columns of that call.  The width of an entity is the number of kept columns in (start, end], from a cumulative sum.
        Pure torch on the tensors' device, no sync.  -> [B,E]: 0 in unused slots, -inf for an entity wider than ``W`` kept
        columns (its event was not computed)."""
        B, S, W, _ = log_post.shape
        b, e, ty = (ents[..., k].long() for k in range(3))
        used = b >= 0
        b, e, ty = b.clamp(0, S - 1), e.clamp(0, S - 1), ty.clamp(min=0)
        cum = torch.cumsum((keep != 0).long(), dim=1)
        w = torch.gather(cum, 1, e) - torch.gather(cum, 1, b)
        flat = log_post.reshape(B, -1)
        got = torch.gather(flat, 1, (b * W + w.clamp(0, W - 1)) * log_post.shape[3] + ty)
        got = torch.where((w >= 0) & (w < W), got, torch.full_like(got, float("-inf")))
        return torch.where(used, got, torch.zeros_like(got))

    @staticmethod
    def chunks_above(log_post, keep, threshold: float = 0.5, max_entities: int = 32) -> dict:
        """The spans of ``chunk_posteriors``' ``log_post`` [B,S,W,n_types] whose posterior is ``>= threshold``, in ``entities``'
        format: entities [B,E,3] int32 (start column, end column, type; -1 in unused slots), log_confidence / confidence [B,E]
        (0 in unused slots), count [B] int32 (may exceed E = max_entities: the first E are stored), ordered by end column, then
        start column, then type.  ``keep`` [B,S]: the kept columns of that call.  Torch ops on the tensors' device, no sync.
        Two different chunks that overlap exclude each other (the later one needs a start inside the earlier one, or they share
        their start and differ in where the first end falls), so with ``threshold > 0.5`` the selection of a sentence cannot
        overlap."""
        if not 0.0 < threshold <= 1.0:
            raise ValueError(f"CRF.chunks_above: threshold={threshold} outside (0, 1]")
        B, S, W, T = log_post.shape
        E, dev = int(max_entities), log_post.device
        kp = keep != 0
        order = torch.cumsum(kp.long(), dim=1) - 1                                  # ordinal of a kept column
        col_of = torch.zeros(B, S + W, dtype=torch.long, device=dev)                # column of an ordinal
        col_of.scatter_(1, torch.where(kp, order, torch.full_like(order, S + W - 1)), torch.arange(S, device=dev).expand(B, S))
        last = (order.clamp(min=0)[:, :, None] + torch.arange(W, device=dev)[None, None, :]).reshape(B, S * W)
        e = torch.gather(col_of, 1, last).reshape(B, S, W, 1).expand(B, S, W, T)
        b = torch.arange(S, device=dev).reshape(1, S, 1, 1).expand(B, S, W, T)
        ty = torch.arange(T, device=dev).reshape(1, 1, 1, T).expand(B, S, W, T)
        sel = log_post >= math.log(threshold)
        key = torch.where(sel, (e * S + b) * T + ty, torch.full_like(e, S * S * T)).reshape(B, -1)
        n = min(E, key.shape[1])
        key, idx = torch.sort(key, dim=1, stable=True)
        key, idx = key[:, :n], idx[:, :n]
        used = key < S * S * T
        ents = torch.stack([key // T // S, key // T % S, key % T], dim=-1)[..., [1, 0, 2]]
        ents = torch.where(used[..., None], ents, torch.full_like(ents, -1)).to(torch.int32)
        lc = torch.where(used, torch.gather(log_post.reshape(B, -1), 1, idx), torch.zeros((), device=dev))
        conf = torch.where(used, torch.exp(lc), torch.zeros_like(lc))
        if n < E:
            pad = E - n
            ents = torch.cat([ents, torch.full((B, pad, 3), -1, dtype=torch.int32, device=dev)], dim=1)
            lc, conf = (torch.cat([x, torch.zeros(B, pad, device=dev)], dim=1) for x in (lc, conf))
        return {"entities": ents, "log_confidence": lc, "confidence": conf, "count": sel.reshape(B, -1).sum(1).to(torch.int32)}

    # ---- per-token tag constraints (csrc/crf_lattice.hip) ----
    def _prep_allowed(self, emissions, allowed, mask, who):
        """``_prep`` plus the tag-set words: ``allowed`` follows ``batch_first`` like the mask and must be int64 [B,S]."""
        if not isinstance(allowed, torch.Tensor) or allowed.dtype != torch.int64:
            raise ValueError(f"{who}: allowed must be an int64 tensor of tag-set words (bit j = tag j allowed), got "
                             f"{getattr(allowed, 'dtype', type(allowed).__name__)}")
        if allowed.dim() != 2:
            raise ValueError(f"{who}: allowed {tuple(allowed.shape)}: expected two dimensions")
        emissions, _, mask = self._prep(emissions, None, mask)
        if not self.batch_first:
            allowed = allowed.transpose(0, 1)
        hip.crf_lattice_check(emissions, allowed, mask, who)
        return emissions.contiguous(), allowed.contiguous(), mask

    def partial_llh(self, emissions, allowed, mask: Optional[torch.Tensor] = None, reduction: str = "none",
                    return_parts: bool = False):
        """Log-probability of the paths that the per-position tag sets permit: ``pllh[b] = logZ_A[b] - logZ[b] <= 0``, the
        marginal likelihood of a partly annotated sentence (mtvaf_crf_lattice_{fwd,bwd}).

        ``allowed`` int64 [B,S] (``batch_first``) or [S,B]: bit ``j`` of a word set = tag ``j`` may be taken at that column; a
        word without any of the low ``num_tags`` bits means "no constraint" and higher bits are ignored
        (``mtvaf_amd.constraints`` builds such words on the device).  ``mask`` is a prefix mask.  A sentence whose sets are
        all full has ``pllh == 0.0`` exactly and contributes exact zeros to every gradient.  Reductions as ``forward``:
        'none' [B], 'sum', 'mean' (over sentences), 'token_mean' (sum / mask.sum()).  ``return_parts``: also ``logz_a`` [B] and
        ``logz`` [B], which carry no gradient."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        em, allowed, mask = self._prep_allowed(emissions, allowed, mask, "CRF.partial_llh")
        pllh, logz_a, logz = engine.CRFLatticeFunction.apply(em, self.start_transitions, self.end_transitions, self.transitions,
                                                             allowed, mask)
        if reduction == "sum":
            pllh = pllh.sum()
        elif reduction == "mean":
            pllh = pllh.mean()
        elif reduction == "token_mean":
            pllh = pllh.sum() / mask.to(pllh.dtype).sum()
        return (pllh, logz_a, logz) if return_parts else pllh

    @torch.no_grad()
    def constrained_marginals(self, emissions, allowed, mask: Optional[torch.Tensor] = None, return_logz: bool = False):
        """Posterior tag probabilities given that the path stays inside the tag sets: ``p(y_t = j | emissions, y in allowed)``,
        [B,S,C] (``batch_first``) or [S,B,C]; exact zeros at disallowed tags and masked columns.  ``return_logz``: also
        ``logz_a`` [B].  ``allowed`` and ``mask`` as for ``partial_llh``.  mtvaf_crf_lattice_marginals; no gradient."""
        em, allowed, mask = self._prep_allowed(emissions, allowed, mask, "CRF.constrained_marginals")
        B, S, C = em.shape
        ws, wsb = hip.crf_lattice_workspace(B, S, C, em.device)
        marg = torch.empty_like(em)
        logz_a = torch.empty(B, dtype=em.dtype, device=em.device) if return_logz else None
        hip.crf_lattice_marginals(em, allowed, mask, self.start_transitions.data, self.end_transitions.data,
                                  self.transitions.data, marg, logz_a, ws, wsb)
        if not self.batch_first:
            marg = marg.transpose(0, 1)
        return (marg, logz_a) if return_logz else marg

    @torch.no_grad()
    def decode_constrained(self, emissions, allowed, mask: Optional[torch.Tensor] = None, return_score: bool = False):
        """Viterbi among the paths the tag sets permit -> (tags int32 [B,S] padded with -1, lengths int32 [B]) on the device
        like ``decode_packed``, with ``return_score`` also the unnormalised score [B] of each path; no host sync.  Equal scores:
        the lowest allowed previous tag, at the end the lowest allowed last tag; with full sets the result is ``decode_packed``'s.
        ``allowed`` and ``mask`` as for ``partial_llh``.  mtvaf_crf_lattice_viterbi."""
        em, allowed, mask = self._prep_allowed(emissions, allowed, mask, "CRF.decode_constrained")
        B, S, _ = em.shape
        tags = torch.empty(B, S, dtype=torch.int32, device=em.device)
        lens = torch.empty(B, dtype=torch.int32, device=em.device)
        score = torch.empty(B, dtype=em.dtype, device=em.device) if return_score else None
        hip.crf_lattice_viterbi(em, allowed, mask, self.start_transitions.data, self.end_transitions.data,
                                self.transitions.data, tags, lens, score)
        return (tags, lens, score) if return_score else (tags, lens)

    # ---- expected cost under the posterior (csrc/crf_risk.hip) ----
    @staticmethod
    def reduce_risk(risk, denominator, reduction: str):
        """``risk`` [B] under the reductions of ``forward``: 'none' [B], 'sum', 'mean' (over sentences), 'token_mean' (sum /
        ``denominator``, the number of columns that count)."""
        if reduction == "none":
            return risk
        if reduction == "sum":
            return risk.sum()
        if reduction == "mean":
            return risk.mean()
        if reduction == "token_mean":
            return risk.sum() / denominator
        raise ValueError(f"invalid reduction: {reduction}")

    @staticmethod
    def hamming_cost(tags, num_tags: int, mask, keep=None):
        """The cost of ``hamming_risk``, batch-first: -> (cost float32 [B,S,C], kept bool [B,S]).  ``kept`` = the unmasked columns
        that ``keep`` (bool [B,S], None: all) does not drop; ``cost[b,t,c] = 1`` for ``c != tags[b,t]`` at kept columns, 0 at
        the gold tag and at every other column.  Torch ops on the tensors' device, no sync; tags outside 0..C-1 (padding
        labels) are clamped, which only matters at columns that do not count."""
        kept = mask != 0
        if keep is not None:
            if tuple(keep.shape) != tuple(mask.shape):
                raise ValueError(f"CRF.hamming_risk: keep {tuple(keep.shape)} does not fit mask {tuple(mask.shape)}")
            kept = kept & (keep != 0)
        cost = kept[..., None].to(torch.float32).repeat(1, 1, num_tags)
        cost.scatter_(2, tags.long().clamp(0, num_tags - 1)[..., None], 0.0)
        return cost, kept

    def _risk(self, em, cost, mask, who):
        hip.crf_risk_check(em, cost, mask, who)
        return engine.CRFRiskFunction.apply(em, self.start_transitions, self.end_transitions, self.transitions, cost.float(),
                                            mask)

    def expected_cost(self, emissions, cost, mask: Optional[torch.Tensor] = None, reduction: str = "none"):
        """The expected value of a column-additive cost under the posterior: ``R[b] = E_{y ~ p(.|x_b)} sum_t cost[b,t,y_t] = sum_t
        sum_c m_t(c) cost[b,t,c]`` over the unmasked columns (mtvaf_crf_risk_{fwd,bwd}), differentiable in the emissions, the
        chain parameters and -- where it requires grad -- ``cost``.  Minimum-risk training, cost-sensitive variants (per-tag
        error weights), distillation terms linear in the marginals.

        ``cost`` is a floating-point tensor of the emissions' shape and follows ``batch_first`` like them; ``mask`` is a prefix
        mask, and cost at masked columns is never read.  A constant added to ``cost[b,t,:]`` moves ``R[b]`` by it and changes
        no gradient.  Reductions as ``forward``: 'none' [B], 'sum', 'mean' (over sentences), 'token_mean' (sum / mask.sum())."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        if not isinstance(cost, torch.Tensor) or not cost.dtype.is_floating_point:
            raise ValueError(f"CRF.expected_cost: cost must be a floating-point tensor, got "
                             f"{getattr(cost, 'dtype', type(cost).__name__)}")
        if tuple(cost.shape) != tuple(emissions.shape):
            raise ValueError(f"CRF.expected_cost: cost {tuple(cost.shape)} does not fit emissions {tuple(emissions.shape)}")
        em, _, mask = self._prep(emissions, None, mask)
        if not self.batch_first:
            cost = cost.transpose(0, 1)
        risk = self._risk(em, cost, mask, "CRF.expected_cost")
        return self.reduce_risk(risk, mask.to(risk.dtype).sum(), reduction)

    def hamming_risk(self, emissions, tags, mask: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                     reduction: str = "token_mean"):
        """The expected number of wrong tags under the posterior, ``sum_t (1 - m_t(tags_t))`` over the columns that count
        ('none' [B], 'sum', 'mean' over sentences), or with 'token_mean' their expected rate: the sum divided by the number
        of columns that count.  ``keep`` bool [B,S] (``batch_first``) or [S,B] drops columns from the count, e.g. those of
        structural labels; a column counts if it is unmasked and kept.  Where no column counts the risk is exactly 0 and so is the
        rate (the denominator is clamped to 1).  The cost is built on the device (``hamming_cost``)."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        em, tags, mask = self._prep(emissions, tags, mask)
        if keep is not None and not self.batch_first:
            keep = keep.transpose(0, 1)
        cost, kept = self.hamming_cost(tags, self.num_tags, mask, keep)
        risk = self._risk(em, cost, mask, "CRF.hamming_risk")
        return self.reduce_risk(risk, kept.to(risk.dtype).sum().clamp(min=1.0), reduction)

    def differentiable_marginals(self, emissions, mask: Optional[torch.Tensor] = None):
        """The values of ``marginals`` -- [B,S,C] (``batch_first``) or [S,B,C], exact zeros at masked steps -- WITH a gradient to
        the emissions and the chain parameters (`engine.CRFMarginalsFunction`: the backward is the risk gradient with the
        incoming cotangent as cost).  For distillation from a teacher's marginals or consistency between two passes.
        ``mask`` is a prefix mask, C at most 64 and S at most 512 as for ``expected_cost``."""
        em, _, mask = self._prep(emissions, None, mask)
        hip.crf_risk_check(em, None, mask, "CRF.differentiable_marginals")
        marg = engine.CRFMarginalsFunction.apply(em, self.start_transitions, self.end_transitions, self.transitions, mask)
        return marg if self.batch_first else marg.transpose(0, 1)

    # ---- path costs with edge terms: expected cost, entropy, KL (csrc/crf_path.hip) ----
    def expected_path_cost(self, emissions, cost=None, edge_cost=None, mask: Optional[torch.Tensor] = None,
                           reduction: str = "none"):
        """The expected value under the posterior of a path cost with a term on every edge: ``R[b] = E_{y ~ p(.|x_b)} [sum_t
        cost[b,t,y_t] + sum_{t>=1} edge_cost[y_{t-1},y_t]]`` over the unmasked columns (mtvaf_crf_path_{fwd,bwd}),
        differentiable in the emissions, the chain parameters and whichever cost requires grad (their gradients are the node
        marginals and the edge marginals summed over columns).  Transition-sensitive risk: penalise ``O -> I-x`` or boundary
        errors.  ``cost`` (emissions' shape, follows ``batch_first``) and ``edge_cost`` [C,C] (row = previous tag) may each be
        None; ``mask`` is a prefix mask.  Reductions as ``forward``.  ``expected_cost`` stays on its own kernels."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        who = "CRF.expected_path_cost"
        if cost is not None:
            if not isinstance(cost, torch.Tensor) or not cost.dtype.is_floating_point:
                raise ValueError(f"{who}: cost must be a floating-point tensor, got {getattr(cost, 'dtype', type(cost).__name__)}")
            if tuple(cost.shape) != tuple(emissions.shape):
                raise ValueError(f"{who}: cost {tuple(cost.shape)} does not fit emissions {tuple(emissions.shape)}")
        em, _, mask = self._prep(emissions, None, mask)
        if cost is not None and not self.batch_first:
            cost = cost.transpose(0, 1)
        hip.crf_path_check(em, cost, edge_cost, mask, who)
        risk = engine.CRFPathFunction.apply(em, self.start_transitions, self.end_transitions, self.transitions,
                                            None if cost is None else cost.float(),
                                            None if edge_cost is None else edge_cost.float(), mask)
        return self.reduce_risk(risk, mask.to(risk.dtype).sum(), reduction)

    def entropy(self, emissions, mask: Optional[torch.Tensor] = None, reduction: str = "none"):
        """The entropy of the posterior over whole tag sequences, ``H[b] = -sum_y p(y|x_b) log p(y|x_b) = logZ - E_p[score]``, in
        nats, with a gradient to the emissions and the chain parameters (`engine.CRFEntropyFunction`: one forward and one
        backward kernel call).  The sequence-level uncertainty beside ``decode_nbest``'s ``p(best path)``; as a loss term,
        entropy minimisation (or, negated, a confidence penalty).  ``0 <= H <= len * log(num_tags)``.  ``mask`` is a prefix
        mask.  Reductions as ``forward``; 'token_mean' divides by the unmasked columns."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        em, _, mask = self._prep(emissions, None, mask)
        hip.crf_path_check(em, None, None, mask, "CRF.entropy")
        h = engine.CRFEntropyFunction.apply(em, self.start_transitions, self.end_transitions, self.transitions, mask)
        return self.reduce_risk(h, mask.to(h.dtype).sum(), reduction)

    def kl_divergence(self, emissions_p, emissions_q, mask: Optional[torch.Tensor] = None, other: Optional["CRF"] = None,
                      reduction: str = "none"):
        """``KL(p || q)[b]`` over whole tag sequences, ``p`` this chain on ``emissions_p`` and ``q`` the chain ``other`` (None:
        this one) on ``emissions_q``, same mask: ``E_p[score_p - score_q] - logZ_p + logZ_q`` (`engine.CRFKLFunction`).
        Gradients flow to both sides -- detach a side (emissions, and for a teacher ``other``'s parameters) and it costs no
        backward call; with shared parameters both contributions accumulate into them.  Distillation from a teacher CRF with
        its own transitions; consistency between two passes.  ``mask`` is a prefix mask.  Reductions as ``forward``."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        q = self if other is None else other
        if q.num_tags != self.num_tags:
            raise ValueError(f"CRF.kl_divergence: other has {q.num_tags} tags, this chain {self.num_tags}")
        if q.transitions.device != self.transitions.device:
            raise ValueError(f"CRF.kl_divergence: other's parameters on {q.transitions.device}, this chain's on "
                             f"{self.transitions.device}")
        if emissions_q.device != emissions_p.device:
            raise ValueError(f"CRF.kl_divergence: emissions_q on {emissions_q.device}, emissions_p on {emissions_p.device}")
        if tuple(emissions_p.shape) != tuple(emissions_q.shape):
            raise ValueError(f"CRF.kl_divergence: emissions_q {tuple(emissions_q.shape)} does not fit emissions_p "
                             f"{tuple(emissions_p.shape)}")
        ep, _, mask = self._prep(emissions_p, None, mask)
        eq = emissions_q.float() if self.batch_first else emissions_q.transpose(0, 1).float()
        hip.crf_path_check(ep, eq, None, mask, "CRF.kl_divergence")
        kl = engine.CRFKLFunction.apply(ep, self.start_transitions, self.end_transitions, self.transitions, eq,
                                        q.start_transitions, q.end_transitions, q.transitions, mask)
        return self.reduce_risk(kl, mask.to(kl.dtype).sum(), reduction)

    def symmetric_kl(self, emissions_a, emissions_b, mask: Optional[torch.Tensor] = None, reduction: str = "mean"):
        """``KL(p_a || p_b)[b] + KL(p_b || p_a)[b]`` over whole tag sequences between this chain's posteriors on two emission
        tensors -- the chain-level consistency term between two passes over one batch.  Both sides share the transitions, so with
        ``D = emissions_a - emissions_b`` the difference of the two path scores is column-additive, ``score_a(y) - score_b(y) =
        sum_t D[t,y_t]``, and ``KL(p_a || p_b) = E_a[sum_t D[t,y_t]] - logZ_a + logZ_b``, ``KL(p_b || p_a) = -E_b[sum_t D[t,y_t]] +
        logZ_a - logZ_b``: both ``logZ`` cancel in the sum,

            symKL = E_{p_a}[sum_t D[t,y_t]] - E_{p_b}[sum_t D[t,y_t]]

        which is two ``expected_cost`` calls with cost ``D`` (against four risk launches and two ``logZ`` for two ``kl_divergence``
        calls).  Gradients reach both emission tensors -- through the posteriors and through the cost -- and the chain
        parameters.  Exactly 0 when both arguments are one tensor.  The limits of ``expected_cost``: at most 64 tags and 512
        columns, ``mask`` a prefix mask.  Reductions as ``forward``: 'none' [B], 'sum', 'mean' (over sentences), 'token_mean'."""
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"invalid reduction: {reduction}")
        if tuple(emissions_a.shape) != tuple(emissions_b.shape):
            raise ValueError(f"CRF.symmetric_kl: emissions_b {tuple(emissions_b.shape)} does not fit emissions_a "
                             f"{tuple(emissions_a.shape)}")
        delta = emissions_a.float() - emissions_b.float()
        skl = self.expected_cost(emissions_a, delta, mask, "none") - self.expected_cost(emissions_b, delta, mask, "none")
        columns = emissions_a.shape[0] * emissions_a.shape[1] if mask is None else mask.ne(0).sum().to(skl.dtype)
        return self.reduce_risk(skl, columns, reduction)

    def decode_deferred(self, emissions, mask: Optional[torch.Tensor] = None) -> DeferredTags:
        """Viterbi on device + asynchronous packed copy to pinned host memory; no host sync here."""
        return self.defer_packed(*self.decode_packed(emissions, mask))

    def defer_packed(self, tags, lens) -> DeferredTags:
        """``decode_deferred``'s second half for tags that are on the device already: tags int32 [B,S] (-1 beyond each length) and
        lens int32 [B] -> the list that fills itself from an asynchronous packed copy."""
        S = tags.shape[1]
        packed = torch.cat([tags, lens[:, None]], dim=1)
        need = packed.numel()
        buf = None
        for i, (t, ev_old) in enumerate(self._host_pool):
            if t.numel() >= need and (ev_old is None or ev_old.query()):
                buf = self._host_pool.pop(i)[0]
                break
        if buf is None:
            buf = torch.empty(max(need, 1 << 14), dtype=packed.dtype, pin_memory=True)
        host = buf[:need].view(packed.shape)
        host.copy_(packed, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        pool = self._host_pool
        out = DeferredTags(host, ev, S, release=lambda: pool.append((buf, ev)) if len(pool) < 8 else None)
        out.device_tags = tags  # for on-device consumers (mtvaf_amd.metrics.EntityScorer): no second launch, no copy
        return out

    def decode(self, emissions, mask: Optional[torch.Tensor] = None) -> List[List[int]]:
        tags, lens = self.decode_packed(emissions, mask)
        packed = torch.cat([tags, lens[:, None]], dim=1).cpu()  # ONE D2H copy
        S = tags.shape[1]
        return [row[:n].tolist() for row, n in zip(packed[:, :S], packed[:, S].tolist())]
