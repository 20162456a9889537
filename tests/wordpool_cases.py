"""Case table, input builders and the restatement of the contract of csrc/wordpool.hip (include/mtvaf_hip.h: mtvaf_word_index,
mtvaf_word_pool_fwd, mtvaf_word_pool_bwd).  Shared by test_wordpool.py (CPU: the restatement against a
brute-force walk, the label helpers) and test_wordpool_gpu.py (the kernels, the model).  Nothing here imports mtvaf_amd: torch on
the host, integers for the index, float64 from the fp32 inputs for the pooling.

The rule (written from the contract, not from the kernel).  len = the leading non-zero entries of the mask.  Token s < len OPENS a
column iff s == 0, map[s] < 0 or map[s] != map[s-1]; a token belongs to the column opened last.  Columns are numbered in order; those
at W and beyond are dropped (col_of_token -1 there), n_cols counts them all the same.  Map entries at s >= len are never read.

The bounds, from the arithmetic the contract pins (u = 2^-24, one fp32 rounding; nothing is fitted to an output):

  * first / last are copies: 0 (torch.equal).
  * mean, forward: n pieces added one after the other in ascending token order in fp32 -- n - 1 roundings, each at most u times a
    partial sum that is at most sum |x_i| in magnitude: (n - 1) u sum |x_i| on the sum, the same over n on the mean -- then ONE
    correctly rounded division, u |y|:    |y - y64| <= (n - 1) u sum |x_i| / n + u |y64| + 2^-149.
    2^-149 (half the spacing of the fp32 subnormals, twice over) covers a quotient that lands in the subnormal range, where a
    rounding is absolute, not relative.
  * mean, backward: dy / (float)n is one correctly rounded division:    |dx - dx64| <= u |dx64| + 2^-149.
  * dead columns, masked tokens, tokens of dropped columns and unselected pieces: exact zeros."""
import torch

U32 = 2.0 ** -24
FLOOR = 2.0 ** -149
MODES = ("first", "last", "mean")
SENTINEL = -77  # pre-fill of the integer outputs: no contract value


def sentence(S, length, pieces, sep=True, garbage=None):
    """One row of token_to_word: [CLS] (-1), then the words -- ``pieces`` is a list of piece counts, or of (word id, piece count)
    pairs, id -1 for an unmapped hole -- cut at the sentence's end, then [SEP] (-1) at length - 1 if ``sep``.  Behind ``length``:
    -1, or ``garbage`` (a torch.Generator): arbitrary integers, negative and huge ones among them."""
    row = [-1] * S
    if garbage is not None:
        row = torch.randint(-(2 ** 31), 2 ** 31 - 1, (S,), generator=garbage).tolist()
    if length == 0:
        return row
    row[0] = -1
    end = length - 1 if sep and length > 1 else length
    s, wid = 1, 0
    for p in pieces:
        w, n = p if isinstance(p, tuple) else (wid, p)
        for _ in range(n):
            if s < end:
                row[s] = w
                s += 1
        if not isinstance(p, tuple):
            wid += 1
    last = row[s - 1] if s > 1 else 0
    while s < end:  # (pieces ran out: the last word goes on, one more piece each)
        row[s] = last if last >= 0 else 0
        s += 1
    if end < length:
        row[end] = -1
    return row


def _random_pieces(gen, total, hi=4):
    out = []
    while sum(out) < total:
        out.append(int(torch.randint(1, hi + 1, (1,), generator=gen)))
    return out


def _case(cid, S, H, rows, W=None):
    """rows: [(length, token_to_word row)]"""
    assert len(rows) <= 4
    return dict(id=cid, S=S, H=H, W=W, lengths=[r[0] for r in rows], map=[r[1] for r in rows])


def _cases():
    g = torch.Generator().manual_seed(4242)
    out = [
        _case("S1-H1-cls-only-and-empty", 1, 1, [(1, sentence(1, 1, [])), (0, sentence(1, 0, [], garbage=g))]),
        _case("S2-H20-cls-sep", 2, 20, [(2, sentence(2, 2, [])), (1, sentence(2, 1, [], garbage=g)), (0, sentence(2, 0, []))]),
        _case("S7-H20-five-pieces-identity-truncated", 7, 20,
              [(7, sentence(7, 7, [5])),                       # one word of 5 pieces
               (4, sentence(7, 4, [1, 1])),                    # every word one piece: the identity
               (7, sentence(7, 7, [1, 5], sep=False))]),       # the word's last piece is the last unmasked token: no [SEP]
        _case("S7-H768-real-row-wider-axis", 7, 768, [(7, sentence(7, 7, [2, 1, 2])), (3, sentence(7, 3, [1], garbage=g))], W=12),
        _case("S64-H64-one-wave", 64, 64,
              [(64, sentence(64, 64, [1] * 62)),                               # identity at the full width of a wave
               (64, sentence(64, 64, [62])),                                   # all mapped tokens in one word
               (40, sentence(64, 40, _random_pieces(g, 40), garbage=g)),       # a garbage map behind the mask
               (0, sentence(64, 0, [], garbage=g))]),
        _case("S65-H768-holes-and-equal-ids-across-a-hole", 65, 768,
              [(65, sentence(65, 65, [(0, 3), (-1, 1), (0, 2), (1, 1), (-1, 2), (2, 4), (2, 1), (3, 50), (4, 3)])),
               (64, sentence(65, 64, _random_pieces(g, 64), garbage=g))]),
        _case("S512-H64-words-across-the-64-token-chunks", 512, 64,
              [(512, sentence(512, 512, _random_pieces(g, 60) + [70, 1, 130] + _random_pieces(g, 300))),
               (300, sentence(512, 300, _random_pieces(g, 300, hi=7), sep=False, garbage=g)),
               (129, sentence(512, 129, [1] * 127))]),
        _case("S64-H20-overflow-W5", 64, 20,
              [(30, sentence(64, 30, _random_pieces(g, 30))), (5, sentence(64, 5, [1, 1, 1])), (4, sentence(64, 4, [2])),
               (64, sentence(64, 64, [1] * 62))], W=5),
        _case("S7-H1-scalar", 7, 1, [(6, sentence(7, 6, [3, 1])), (7, sentence(7, 7, [(5, 2), (-1, 1), (5, 2)]))]),
    ]
    return out


CASES = _cases()
IDS = [c["id"] for c in CASES]


def make_index_inputs(case):
    """-> attention_mask [B,S] uint8 (a prefix mask), token_to_word [B,S] int32, W"""
    S = case["S"]
    mask = torch.zeros(len(case["lengths"]), S, dtype=torch.uint8)
    for b, n in enumerate(case["lengths"]):
        mask[b, :n] = 1
    return mask, torch.tensor(case["map"], dtype=torch.int32).view(len(case["lengths"]), S), case["W"] or S


def make_x(case, seed=0, width=None):
    """x [B,S,H] fp32 (width: [B,W,H], a dy), values of mixed magnitude so that sums round"""
    gen = torch.Generator().manual_seed(100 + seed)
    B, S, H = len(case["lengths"]), case["S"] if width is None else width, case["H"]
    return torch.randn(B, S, H, generator=gen) * torch.exp2(torch.randint(-6, 7, (B, S, 1), generator=gen).float())


def index_reference(mask, t2w, W):
    """The rule, vectorised, in integers -> dict of the six outputs (int32 / uint8, as the kernel's)."""
    B, S = mask.shape
    live = torch.cumprod((mask != 0).long(), dim=1).bool()
    m = torch.where(live, t2w.long(), torch.full((), -1, dtype=torch.long))
    prev = torch.cat([torch.full((B, 1), -1, dtype=torch.long), m[:, :-1]], dim=1)
    pos = torch.arange(S)[None, :].expand(B, S)
    opens = live & ((pos == 0) | (m < 0) | (m != prev))
    col = torch.cumsum(opens.long(), dim=1) - 1
    kept = live & (col < W)
    col_start = torch.zeros(B, W, dtype=torch.long)
    col_len = torch.zeros(B, W, dtype=torch.long)
    word_id = torch.full((B, W), -1, dtype=torch.long)
    bi = torch.arange(B)[:, None].expand(B, S)
    first = opens & kept
    col_start[bi[first], col[first]] = pos[first]
    word_id[bi[first], col[first]] = m[first].clamp_min(-1)
    col_len.index_put_((bi[kept], col[kept]), torch.ones((), dtype=torch.long), accumulate=True)
    i32 = lambda t: t.to(torch.int32)
    return dict(col_start=i32(col_start), col_len=i32(col_len),
                col_of_token=i32(torch.where(kept, col, torch.full((), -1, dtype=torch.long))),
                word_mask=(col_len > 0).to(torch.uint8), word_id=i32(word_id), n_cols=i32(opens.sum(1)))


def index_brute(mask, t2w, W):
    """The rule once more, token by token in Python."""
    B, S = mask.shape
    out = dict(col_start=torch.zeros(B, W, dtype=torch.int32), col_len=torch.zeros(B, W, dtype=torch.int32),
               col_of_token=torch.full((B, S), -1, dtype=torch.int32), word_mask=torch.zeros(B, W, dtype=torch.uint8),
               word_id=torch.full((B, W), -1, dtype=torch.int32), n_cols=torch.zeros(B, dtype=torch.int32))
    for b in range(B):
        length = 0
        while length < S and int(mask[b, length]) != 0:
            length += 1
        col = -1
        for s in range(length):
            m = int(t2w[b, s])
            if s == 0 or m < 0 or m != int(t2w[b, s - 1]):
                col += 1
                if col < W:
                    out["col_start"][b, col] = s
                    out["word_id"][b, col] = m if m >= 0 else -1
                    out["word_mask"][b, col] = 1
            if col < W:
                out["col_len"][b, col] += 1
                out["col_of_token"][b, s] = col
        out["n_cols"][b] = col + 1
    return out


def pool_reference(x, idx, mode):
    """-> y64 [B,W,H] float64 and tol [B,W,H]: the bound of the module docstring (0 for the copies and on dead columns)."""
    B, S, H = x.shape
    W = idx["col_start"].shape[1]
    x64 = x.double()
    y = torch.zeros(B, W, H, dtype=torch.float64)
    tol = torch.zeros(B, W, H, dtype=torch.float64)
    for b in range(B):
        for w in range(W):
            s0, n = int(idx["col_start"][b, w]), int(idx["col_len"][b, w])
            if n == 0:
                continue
            if mode == "first":
                y[b, w] = x64[b, s0]
            elif mode == "last":
                y[b, w] = x64[b, s0 + n - 1]
            else:
                y[b, w] = x64[b, s0:s0 + n].sum(0) / n
                tol[b, w] = (n - 1) * U32 * x64[b, s0:s0 + n].abs().sum(0) / n + U32 * y[b, w].abs() + FLOOR
    return y, tol


def pool_bwd_reference(dy, idx, mode):
    """-> dx64 [B,S,H] float64 and tol: one rounding for the mean, 0 otherwise."""
    B, W, H = dy.shape
    S = idx["col_of_token"].shape[1]
    dy64 = dy.double()
    dx = torch.zeros(B, S, H, dtype=torch.float64)
    tol = torch.zeros(B, S, H, dtype=torch.float64)
    for b in range(B):
        for s in range(S):
            c = int(idx["col_of_token"][b, s])
            if c < 0:
                continue
            s0, n = int(idx["col_start"][b, c]), int(idx["col_len"][b, c])
            if mode == "mean":
                dx[b, s] = dy64[b, c] / n
                tol[b, s] = (U32 * dx[b, s].abs() + FLOOR) if n > 1 else 0.0
            elif s == (s0 if mode == "first" else s0 + n - 1):
                dx[b, s] = dy64[b, c]
    return dx, tol


def eager_pool(x, idx, mode):
    """The pooling as differentiable torch ops in x's dtype (float64 in the model tests' hand composition): x [B,S,H] -> [B,W,H]."""
    B, S, H = x.shape
    W = idx["col_start"].shape[1]
    start, n = idx["col_start"].to(x.device).long(), idx["col_len"].to(x.device).long()
    live = (n > 0)[..., None]
    if mode in ("first", "last"):
        at = start if mode == "first" else (start + n - 1).clamp_min(0)
        return torch.where(live, x.gather(1, at[..., None].expand(B, W, H)), torch.zeros((), dtype=x.dtype, device=x.device))
    col = idx["col_of_token"].to(x.device).long()
    onehot = (col[:, None, :] == torch.arange(W, device=x.device)[None, :, None]).to(x.dtype)  # [B,W,S]
    xz = torch.where((col >= 0)[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    return torch.bmm(onehot, xz) / n.clamp_min(1)[..., None].to(x.dtype)


def excess(got, ref, tol):
    """max |got - ref| / tol over the elements (0 where the error is 0; inf where got is not finite or errs where tol is 0)"""
    got, ref = got.detach().double().cpu(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    return float(q.max()) if q.numel() else 0.0
