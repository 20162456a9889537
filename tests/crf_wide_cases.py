"""Inputs and the Viterbi acceptance rule shared by the wide-tag CRF tests (test_crf_wide.py on the CPU,
test_crf_wide_gpu.py on the GPU): the CPU file checks that the float32 oracle alone meets the rule on every draw the GPU
file decodes, so the rule's cap is never spent on a draw that the reference itself cannot rank."""
import torch

from oracle import mtvaf_oracle as O

# (B, S, C, scale): scale > 1 spreads emissions / transitions over tens of nats, scale < 0 punches holes in the mask
FIXED = [(4, 5, 17, 1), (32, 128, 17, 1), (32, 128, 33, 1), (32, 128, 64, 1), (3, 512, 64, 1), (3, 512, 21, 1),
         (2, 1, 64, 1), (6, 128, 40, 6), (6, 128, 64, 6), (4, 66, 48, -1), (4, 200, 64, -1)]
N_RANDOM = 30
# brute-force known answers: (B, S, C, seed, lengths)
BRUTE = [(3, 5, 17, 77, [4, 3, 1]), (2, 4, 64, 78, [3, 2])]


def crf_inputs(B, S, C, seed, lengths=None):
    gnr = torch.Generator().manual_seed(seed)
    em = torch.randn(B, S, C, generator=gnr)
    start, end = torch.rand(C, generator=gnr) - 0.5, torch.rand(C, generator=gnr) - 0.5
    trans = torch.rand(C, C, generator=gnr) - 0.5
    if lengths is None:
        lengths = [S] + [int(x) for x in torch.randint(1, S + 1, (B - 1,), generator=gnr)]
    mask = torch.zeros(B, S, dtype=torch.uint8)
    for b, Lb in enumerate(lengths):
        mask[b, :Lb] = 1
    tags = torch.randint(0, C, (B, S), generator=gnr)
    return em, tags, mask, start, end, trans


def fixed_case(B, S, C, scale):
    em, tags, mask, start, end, trans = crf_inputs(B, S, C, 3 + S + 1000 * C)
    if scale > 1:
        em, trans = em * scale, trans * 4 * scale
    if scale < 0:
        holes = torch.rand(B, S, generator=torch.Generator().manual_seed(5)) < 0.2
        holes[:, 0] = False
        mask = mask * (~holes).to(mask.dtype)
    return em, tags, mask, start, end, trans


def random_draws():
    """N_RANDOM draws with 17 <= C <= 64, 1 <= S <= 512, holes in every third draw: (tag, inputs)."""
    gnr = torch.Generator().manual_seed(4048)
    for it in range(N_RANDOM):
        B = int(torch.randint(1, 7, (1,), generator=gnr))
        S = int(torch.randint(1, 513, (1,), generator=gnr))
        C = int(torch.randint(17, 65, (1,), generator=gnr))
        em, tags, mask, start, end, trans = crf_inputs(B, S, C, 5000 + it)
        if it % 3 == 0 and S > 2:
            holes = torch.rand(B, S, generator=gnr) < 0.15
            holes[:, 0] = False
            mask = mask * (~holes).to(mask.dtype)
        yield f"draw {it}: B={B} S={S} C={C}", (em, tags, mask, start, end, trans)


def viterbi_cap(n_sentences):
    """How many paths a test may accept by the near-tie clause: max(1, floor(1 % of its sentences))."""
    return max(1, n_sentences // 100)


def viterbi_near_ties(got, em, mask, start, end, trans):
    """Checks decoded paths against the float64 oracle.  A path is accepted if it equals the oracle's, or if its float64
    score is within delta = 2^-24 * L * |s*| of the best score s* (L accumulated float32 roundings at the best score's
    magnitude: such a path cannot be ranked against the best in float32).  Returns (number accepted by the second clause,
    list of (sentence, reason) failures)."""
    emd, sd, ed, td = (t.double() for t in (em, start, end, trans))
    want = O.crf_decode(emd, mask, sd, ed, td)
    B, S, _ = em.shape
    near, bad = 0, []
    for b, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        if len(g) != len(w) or any(not 0 <= x < em.shape[2] for x in g):
            bad.append((b, f"length {len(g)} vs {len(w)} or tag out of range"))
            continue
        L = len(w)

        def score(p):
            t = torch.tensor([list(p) + [0] * (S - L)], dtype=torch.long)
            return float(O.crf_sequence_score(emd[b:b + 1], t, mask[b:b + 1], sd, ed, td)[0])
        s_star, s = score(w), score(g)
        delta = 2.0 ** -24 * L * abs(s_star)
        if s_star - s <= delta:
            near += 1
        else:
            bad.append((b, f"score gap {s_star - s:.3e} > delta {delta:.3e}"))
    return near, bad
