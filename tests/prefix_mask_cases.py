"""Cases of the per-sentence prefix-slot mask and their float64 restatement, shared by test_prefix_mask.py on the
CPU and test_prefix_mask_gpu.py on the GPU.  No GPU import here.

The restatement is attn_cases.reference -- plain float64 torch over the [B, P + S] additive mask, gradients by autograd -- on
`attn_cases.Case` objects whose ``masked_prefix`` holds the pattern; layouts are the C-ABI's (see attn_cases.py).  What this file
adds: the shapes and patterns of the issue, the packed-row bookkeeping of a case WITH masked prefix slots (attn_cases.kept_rows
refuses those: before the mask existed the packed layout could not run them) and the additive [B, P] mask the packed launches take.

Shapes: NH = 2 (H = 128), B = 3, sentence lengths (5, S, 1) -- the longest-first launch order (1, 0, 2) is not the batch order, and
a one-token sentence exists.  (P, S): (4, 16) one key tile; (16, 70) prefix and text share tile 0 and a second tile exists;
(36, 128) the headline P; (100, 30) a prefix longer than a key tile, whose first tile holds prefix slots only -- the launchers
take any P >= 0 (attn_check), so the pair is in."""
import functools

import numpy as np
import torch

import attn_cases as AC

B, NH = 3, 2
SHAPES = [(4, 16), (16, 70), (36, 128), (100, 30)]
PATTERNS = ["none", "one_full", "holes", "last"]
FULL = 2  # the sentence that loses every slot in "one_full": the one-token sentence -- a single key remains


def lengths(S):
    return (5, S, 1)


def masked_slots(pattern, P):
    """((sentence, slot), ...) of a pattern."""
    if pattern == "none":
        return ()
    if pattern == "one_full":
        return tuple((FULL, t) for t in range(P))
    if pattern == "last":
        return tuple((b, P - 1) for b in range(B))
    assert pattern == "holes"  # a different set per sentence: every third slot / the first half / all but the last slot
    return (tuple((0, t) for t in range(P) if t % 3 == 1) + tuple((1, t) for t in range(P // 2))
            + tuple((2, t) for t in range(P - 1)))


@functools.lru_cache(maxsize=None)
def case(P, S, pattern):
    return AC.Case(f"pm_p{P}_s{S}_{pattern}", B=B, S=S, P=P, NH=NH, lengths=lengths(S), masked_prefix=masked_slots(pattern, P),
                   seed=100 + P)  # (the seed does not depend on the pattern: the patterns of a shape share their operands)


CASES = [case(P, S, pat) for P, S in SHAPES for pat in PATTERNS]


def pmask_of(c):
    """[B, P] additive fp32: 0 = slot present, -10000 = absent -- the prefix columns of the padded layout's addmask."""
    return ((1.0 - AC.mask_of(c)[:, :c.P]) * -10000.0).contiguous()


def slot_masked(c):
    """[B, P] bool."""
    return AC.mask_of(c)[:, :c.P] == 0


def kept_rows(c):
    return torch.tensor([b * c.S + s for b, n in enumerate(c.lengths) for s in range(n)])


def cu_plain(c):
    return torch.tensor(np.concatenate([[0], np.cumsum(c.lengths)]), dtype=torch.int32)


def cu_ordered(c):
    """cu [2B+1] of the ordered launch (attn_cases.cu_ordered): cu[0] = -1, the offsets, then the sentences longest first."""
    order = sorted(range(c.B), key=lambda b: (-c.lengths[b], b))
    out = torch.cat([cu_plain(c), torch.tensor(order, dtype=torch.int32)])
    out[0] = -1
    return out


def live_queries(c):
    """[B, NH, S] bool: the queries a packed launch computes."""
    q = torch.zeros(c.B, c.S, dtype=torch.bool)
    q.view(-1)[kept_rows(c)] = True
    return q[:, None, :].expand(c.B, c.NH, c.S)


@functools.lru_cache(maxsize=None)
def reference(c, p=0.0, bf16=False):
    """The float64 restatement of a case, computed once and shared (nobody writes into it).  dctx is zero behind each sentence's
    last token (a packed launch has no padded queries), dropout by the replicated keep mask."""
    keep = AC.keep_mask(AC.SEED, AC.OFFSET, c.B, c.NH, c.S, c.T, p) if p else None
    return AC.reference(c, keep=keep, p=p, bf16=bf16, zero_tail=True)
