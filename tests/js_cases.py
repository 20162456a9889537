"""Case table and float64 restatement of the span model's cutoff consistency term (reference modules/train.py:523-538,
cal_cut_loss / js_div), shared by test_js_consistency.py (CPU) and test_js_consistency_gpu.py."""
import math

import torch
import torch.nn.functional as F

# (B, M, C, logit scale s, perturbation d):  x = s * randn,  y = x + d * s * randn
CASES = [(1, 1, 4, 1, 1), (2, 20, 4, 1, 1), (2, 20, 4, 3, 1), (3, 7, 1, 3, 1), (5, 33, 4, 3, 1), (2, 64, 4, 3, 1),
         (2, 65, 3, 3, 1), (1, 1000, 4, 3, 1), (32, 20, 4, 3, 1), (2, 20, 4, 3, 0.01), (2, 20, 4, 3, 0), (2, 20, 4, 40, 1),
         (2, 130, 4, 60, 1), (1, 1024, 16, 3, 1)]
UPSTREAM = 1.7   # factor in front of js when the gradients are taken


def case_id(case):
    return "B{}-M{}-C{}-s{}-d{}".format(*case)


def make_logits(B, M, C, s, d, seed=None):
    """-> x, y fp32 [B,M,C]"""
    g = torch.Generator().manual_seed(1000 * B + 10 * M + C if seed is None else seed)
    x = s * torch.randn(B, M, C, generator=g)
    y = x + d * s * torch.randn(B, M, C, generator=g)
    return x, y


def prefix_mask(M, counts):
    """[B,M] int64: the first counts[b] slots of sentence b are live"""
    return (torch.arange(M)[None, :] < torch.tensor(counts)[:, None]).long()


def masked_cases():
    """-> [(id, x, y, mask)]"""
    x0, y0 = make_logits(3, 20, 4, 3, 1, seed=71)
    x1, y1 = make_logits(2, 65, 3, 3, 1, seed=72)
    alternate = (torch.arange(65) % 2 == 0).long()[None, :].expand(2, -1).contiguous()
    return [("prefix-20-6-0", x0, y0, prefix_mask(20, [20, 6, 0])), ("every-other-slot", x1, y1, alternate)]


def js_ref(x, y):
    """The reference's arithmetic, transcribed literally, in float64."""
    p = torch.softmax(x.double() + 1e-10, 1)
    q = torch.softmax(y.double() + 1e-10, 1)
    m = (p + q) / 2
    return (F.kl_div(p.log(), m, reduction='batchmean') + F.kl_div(q.log(), m, reduction='batchmean')) / 2


def js_ref_masked(x, y, mask):
    """The same formula in log space over the live slots only (mask [B,M], non-zero = live); sentences without a live slot
    are skipped, the divisor stays B."""
    B = x.shape[0]
    total = x.new_zeros((), dtype=torch.float64)
    for b in range(B):
        live = mask[b] != 0
        if not bool(live.any()):
            continue
        lp = torch.log_softmax(x[b].double()[live], 0)
        lq = torch.log_softmax(y[b].double()[live], 0)
        lm = torch.logaddexp(lp, lq) - math.log(2.0)
        total = total + (lm.exp() * (2 * lm - lp - lq)).sum()
    return total / (2 * B)


def ref_with_grads(x, y, mask=None):
    """-> (js, d(UPSTREAM * js)/dx, d(UPSTREAM * js)/dy), all float64"""
    xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
    js = js_ref(xd, yd) if mask is None else js_ref_masked(xd, yd, mask)
    gx, gy = torch.autograd.grad(UPSTREAM * js, (xd, yd))
    return js.detach(), gx, gy
