"""An independent reference of the action sampler's draws (numpy only, CPU) -- TEST INFRASTRUCTURE ONLY.

Written from the Philox paper (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11)
and from include/marlmaze.h's description of mm_sample, not from the device code:

* the draw of row ``row`` at (seed, offset) is Philox4x32-10 of counter (offset & 0xFFFFFFFF, offset >> 32, row, 0)
  under key (seed & 0xFFFFFFFF, seed >> 32);
* ``u = (word >> 8) / 2**24``, output word 0 for the move, word 1 for the mark;
* the move is the first legal index j with ``u_move * sum < cumsum_j`` over ``p = exp(l - max)`` of the legal
  entries (move 4 where no move is legal), the mark is allowed and ``u_mark < sigmoid(mark_logit)``.

``replay`` works in float64 and also says how far each draw was from its decision boundary (the margins): a
kernel that rounds in fp32 may differ from it only where a margin is tiny.  ``replay_f32`` does every operation
in float32, for inputs whose fp32 arithmetic is exact by construction.

The second half builds the inputs of tests/test_cpu_sampler_ref.py and tests/test_gpu_sampler_replay.py (the CPU
file establishes on the reference that the GPU file's bounds hold for exactly these arrays) and the frequency
checks both apply.
"""
from collections import namedtuple

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

Replay = namedtuple("Replay", "move mark legal move_margin mark_margin logp")


# ---------------------------------------------------------------------------
# Philox4x32-10
# ---------------------------------------------------------------------------
def philox4x32_10(ctr4, key2):
    """Philox4x32-10: ctr4 [..., 4] and key2 [..., 2] (or [2]) of uint32 words held in uint64 -> [..., 4].

    One round (the paper's figure 1 with N = 4): (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, the new counter is
    (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between rounds."""
    c = np.asarray(ctr4, dtype=np.uint64)
    k = np.asarray(key2, dtype=np.uint64)
    assert c.shape[-1] == 4 and k.shape[-1] == 2 and (c <= M32).all() and (k <= M32).all()
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1)


def _rows(rows):
    return np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64)


def words(seed, offset, rows):
    """The four output words of every row's draw: rows an int (rows 0 .. rows - 1) or an array of row numbers."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    r = _rows(rows)
    ctr = np.zeros(r.shape + (4,), np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = offset & 0xFFFFFFFF, offset >> 32, r
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def uniforms(seed, offset, rows):
    """(u_move, u_mark) in [0, 1 - 2^-24], float64 (24-bit fractions: exact, also as float32)."""
    w = words(seed, offset, rows)
    u = (w >> np.uint64(8)).astype(np.float64) / 2.0**24
    return u[..., 0], u[..., 1]


# ---------------------------------------------------------------------------
# The draw
# ---------------------------------------------------------------------------
def _replay(move_logits, mark_logits, masks, seed, offset, rows, ft):
    ml = np.asarray(move_logits).astype(ft).reshape(-1, 5)
    M = ml.shape[0]
    kl = np.asarray(mark_logits).astype(ft).reshape(M)
    mk = np.asarray(masks).reshape(M, 6) != 0
    um, uk = (u.astype(ft) for u in uniforms(seed, offset, M if rows is None else rows))
    legal = mk[:, :5].any(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = np.where(mk[:, :5], ml, ft(-np.inf)).max(1, keepdims=True)
        p = np.where(mk[:, :5], np.exp(np.where(mk[:, :5], ml - mx, ft(0))), ft(0)).astype(ft)
        # the running sum over the legal entries in index order (illegal entries add an exact 0)
        cum = np.zeros((M, 5), ft)
        acc = np.zeros(M, ft)
        for j in range(5):
            acc = (acc + p[:, j]).astype(ft)
            cum[:, j] = acc
        total = cum[:, 4]
        target = (um * total).astype(ft)
        hit = mk[:, :5] & (target[:, None] < cum)
        last = 4 - np.argmax(mk[:, :5][:, ::-1], 1)  # rounding left the target at the whole sum: the last legal
        move = np.where(hit.any(1), np.argmax(hit, 1), last)
        move = np.where(legal, move, 4)
        dist = np.where(mk[:, :5], np.abs(target[:, None] - cum) / total[:, None], np.inf)
        move_margin = np.where(legal, dist.min(1), np.inf)
        pm = (ft(1) / (ft(1) + np.exp(-kl))).astype(ft)
        mark = mk[:, 5] & (uk < pm)
        mark_margin = np.where(mk[:, 5], np.abs(uk - pm), np.inf)
    act = np.stack([move, mark.astype(np.int64)], 1)
    return Replay(move, mark.astype(np.int64), legal, move_margin.astype(np.float64),
                  mark_margin.astype(np.float64), logp64(ml, kl, mk, act))


def replay(move_logits, mark_logits, masks, seed, offset, rows=None):
    """The draws of M rows in float64: move_logits [M, 5], mark_logits [M] or [M, 1], masks [M, 6].

    Returns Replay(move, mark, legal, move_margin, mark_margin, logp), one entry per row:
    move_margin = min over the legal j of |u_move * sum - cumsum_j| / sum (inf without a legal move),
    mark_margin = |u_mark - sigmoid| (inf where the mark is not allowed), logp the fp64 log-prob of (move, mark)
    (NaN without a legal move).  rows: the rows' numbers where they are not 0 .. M - 1."""
    return _replay(move_logits, mark_logits, masks, seed, offset, rows, np.float64)


def replay_f32(move_logits, mark_logits, masks, seed, offset, rows=None):
    """``replay`` with every operation of the draw in float32 (the log-prob stays fp64)."""
    return _replay(move_logits, mark_logits, masks, seed, offset, rows, np.float32)


def logp64(move_logits, mark_logits, masks, actions):
    """The fp64 log-prob of actions [M, 2] = (move, mark): log-softmax over the legal moves plus log sigmoid(+-
    mark logit) where the mark is allowed; NaN for a row without a legal move."""
    ml = np.asarray(move_logits, dtype=np.float64).reshape(-1, 5)
    M = ml.shape[0]
    kl = np.asarray(mark_logits, dtype=np.float64).reshape(M)
    mk = np.asarray(masks).reshape(M, 6) != 0
    a = np.asarray(actions).astype(np.int64).reshape(M, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(mk[:, :5], ml, -np.inf)
        mx = m.max(1, keepdims=True)
        lsm = m - mx - np.log(np.exp(m - mx).sum(1, keepdims=True))
        lp = lsm[np.arange(M), a[:, 0]]
        logsig = np.where(a[:, 1] != 0, -np.logaddexp(0.0, -kl), -np.logaddexp(0.0, kl))
    lp = lp + np.where(mk[:, 5], logsig, 0.0)
    lp[~mk[:, :5].any(1)] = np.nan
    return lp


def probs64(move_logits, mark_logits, masks):
    """fp64 (softmax over the legal moves [M, 5], P(mark = 1) [M]: sigmoid where allowed, else 0)."""
    ml = np.asarray(move_logits, dtype=np.float64).reshape(-1, 5)
    M = ml.shape[0]
    kl = np.asarray(mark_logits, dtype=np.float64).reshape(M)
    mk = np.asarray(masks).reshape(M, 6) != 0
    m = np.where(mk[:, :5], ml, -np.inf)
    e = np.exp(m - m.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True), np.where(mk[:, 5], 1.0 / (1.0 + np.exp(-kl)), 0.0)


# ---------------------------------------------------------------------------
# The shared inputs of the CPU and the GPU test file
# ---------------------------------------------------------------------------
MOVE_MARGIN, MARK_MARGIN = 1e-5, 1e-6  # a draw nearer to a boundary than this may round the other way in fp32
MAX_EXCLUDED = 1e-3  # share of rows that may be that near
RTOL, ATOL = 1e-5, 1e-6  # the sampler's log-prob bar (tests/test_gpu_rl.py)

# seed 11, row 0: offsets whose draw is an extreme uniform (found by search once; the CPU test checks them)
EDGE_OFFSETS = {  # name: (offset, output word, its value, the uniform)
    "move_max": (858091, 0, 0xFFFFFFF4, 1 - 2.0**-24),
    "move_zero": (49916316, 0, 0x00000061, 0.0),
    "mark_max": (7571245, 1, 0xFFFFFFD9, 1 - 2.0**-24),
    "mark_zero": (7508461, 1, 0x000000E4, 0.0),
}
EDGE_SEED = 11

# (seed, offset, offset_dev): high words of the key and of the counter live, a low word of all ones / of zero, and
# (the fused head only) a device base whose sum with the offset carries into the high word
GENERAL_M = 70001
GENERAL_CASES = [
    (11, 5, None),
    (0x4F1BBCDCBFA53E0A, 2**32 - 1, None),
    (11, 2**32, None),
    (2**63 - 25, 2**40 + 7, None),
]
DEVICE_BASE_CASE = (2**63 - 25, 2**32 - 2, 5)


def general_inputs(M=GENERAL_M):
    """move logits [M, 5] and mark logits [M] ~ N(0, 2) in fp32, masks [M, 6] u8 with P(1) = 0.6; rows 0 .. 4 as
    tests/test_gpu_eval.py::_head_inputs forces them: all legal, one legal move, mark disallowed, no legal move,
    moves (0, 3, 4)."""
    rng = np.random.default_rng(20240 + M)
    ml = rng.normal(0, 2, (M, 5)).astype(np.float32)
    kl = rng.normal(0, 2, M).astype(np.float32)
    mk = rng.random((M, 6)) < 0.6
    mk[0] = True
    if M > 1:
        mk[1] = [False, False, True, False, False, True]
    if M > 4:
        mk[2, 5] = False
        mk[3, :5] = False
        mk[4] = [True, False, False, True, True, True]
    return ml, kl, mk.astype(np.uint8)


def identity_head(move_logits, mark_logits, K=8):
    """(h [M, K], w [6, K], b [6]) whose head logits h w^T + b are the given ones exactly: h = [logits | 0],
    w = [I | 0], b = 0 (every product is x * 1 or x * 0, every sum adds zeros)."""
    M = move_logits.shape[0]
    h = np.zeros((M, K), np.float32)
    h[:, :5] = move_logits
    h[:, 5] = np.asarray(mark_logits).reshape(M)
    w = np.zeros((6, K), np.float32)
    w[np.arange(6), np.arange(6)] = 1.0
    return h, w, np.zeros(6, np.float32)


def exact_inputs(M, level):
    """All six mask bytes 1, five equal move logits ``level``, mark logit 0: p_j = 1, sum = 5, target = fl(u * 5)
    and sigmoid = 0.5 are exact fp32 operations, so replay_f32 predicts every row."""
    return np.full((M, 5), level, np.float32), np.zeros(M, np.float32), np.ones((M, 6), np.uint8)


def bias_head(M, move_logits5, mark_logit, K=8):
    """(h, w, b) with h = 0 and the logits as biases: every row's head logits are exactly the biases."""
    b = np.concatenate([np.asarray(move_logits5, np.float32).reshape(5), np.float32([mark_logit])])
    w = np.random.default_rng(K).normal(0, 1, (6, K)).astype(np.float32)
    return np.zeros((M, K), np.float32), w, b


# the frequency test: 64 classes of 8,192 rows each in one launch
FREQ_CLASSES, FREQ_ROWS = 64, 8192
FREQ_SEED, FREQ_OFFSET = 0x6A09E667F3BCC908, 2**33 + 17  # the first pair tried
FREQ_MIN_DRAWS = 100


def freq_inputs():
    """64 (move logits, mark logit, mask) classes drawn once: logits N(0, 2), the mark logit uniform in [-3, 3],
    masks P(1) = 0.6 with at least one legal move; classes 0 .. 5 forced to one, two and five legal moves (two
    each), class 6 the mark disallowed.  Returns per-class (ml [64, 5], kl [64], mk [64, 6]) and the per-row
    arrays of the launch (class c = rows 8192 c .. 8192 c + 8191)."""
    rng = np.random.default_rng(64)
    C = FREQ_CLASSES
    ml = rng.normal(0, 2, (C, 5)).astype(np.float32)
    kl = rng.uniform(-3, 3, C).astype(np.float32)
    mk = rng.random((C, 6)) < 0.6
    none = ~mk[:, :5].any(1)
    mk[none, rng.integers(0, 5, none.sum())] = True
    mk[0, :5] = [False, False, False, True, False]
    mk[1, :5] = [True, False, False, False, False]
    mk[2, :5] = [False, True, False, False, True]
    mk[3, :5] = [True, False, True, False, False]
    mk[4, :5] = mk[5, :5] = True
    mk[:6, 5] = True
    mk[6, 5] = False
    mk = mk.astype(np.uint8)
    rep = lambda x: np.repeat(x, FREQ_ROWS, axis=0)  # noqa: E731
    return (ml, kl, mk), (rep(ml), rep(kl), rep(mk))


def freq_bound(p, n):
    return 5.0 * np.sqrt(p * (1.0 - p) / n) + 1.0 / n


def frequency_report(classes, actions, logp):
    """The frequency checks of one 64 x 8192-row launch: actions [M, 2], logp [M] (the sampler's per-row
    log-prob, fp32 or fp64).  Returns (violations, worst): violations a list of strings (empty = pass), worst the
    largest |deviation| / bound of each of the three checks.  Per class, n = 8192, and per cell (move = 0 .. 4,
    mark = 1) with p64 from the fp64 softmax / sigmoid:

    1. |freq - p64| <= 5 sqrt(p64 (1 - p64) / n) + 1 / n;
    2. the cell's probability AS STORED against freq, same bound, where the cell has >= 100 draws.  A row's
       log-prob is that of its (move, mark) pair, constant over the rows of a pair, so the stored probability of
       "move = j" is sum over the marks m seen with j of exp(mean logp of the rows (j, m)), and that of "mark = 1"
       the same sum over the moves seen with it (a pair never drawn adds its -- tiny -- mass to neither side);
    3. |P(move = j, mark = 1) - P(move = j) P(mark = 1)| <= 5 sigma, sigma^2 = p_j (1 - p_j) p_m (1 - p_m) / n:
       the variance of that difference of frequencies when the two draws are independent."""
    ml, kl, mk = classes
    n = FREQ_ROWS
    pmove, pmark = probs64(ml, kl, mk)
    a = np.asarray(actions).astype(np.int64).reshape(FREQ_CLASSES, n, 2)
    lp = np.asarray(logp, dtype=np.float64).reshape(FREQ_CLASSES, n)
    bad, worst = [], [0.0, 0.0, 0.0]

    def check(k, what, dev, bound):
        ratio = dev / bound if bound > 0 else (0.0 if dev == 0 else np.inf)
        worst[k] = max(worst[k], ratio)
        if not dev <= bound:
            bad.append(f"{what}: |dev| {dev:.3g} > bound {bound:.3g}")

    for c in range(FREQ_CLASSES):
        pair = np.zeros((5, 2))  # draws of (move, mark)
        np.add.at(pair, (a[c, :, 0], a[c, :, 1]), 1)
        stored = np.zeros((5, 2))  # exp(mean logp) of the pair's rows
        for j in range(5):
            for m in range(2):
                if pair[j, m]:
                    stored[j, m] = np.exp(lp[c][(a[c, :, 0] == j) & (a[c, :, 1] == m)].mean())
        cells = [(f"class {c} move {j}", pair[j].sum(), pmove[c, j], stored[j].sum()) for j in range(5)]
        cells.append((f"class {c} mark", pair[:, 1].sum(), pmark[c], stored[:, 1].sum()))
        for what, cnt, p, st in cells:
            check(0, what + " freq", abs(cnt / n - p), freq_bound(p, n))
            if cnt >= FREQ_MIN_DRAWS:
                check(1, what + " stored", abs(st - cnt / n), freq_bound(p, n))
        f1 = pair[:, 1].sum() / n
        for j in range(5):
            sig = np.sqrt(pmove[c, j] * (1 - pmove[c, j]) * pmark[c] * (1 - pmark[c]) / n)
            check(2, f"class {c} move {j} x mark", abs(pair[j, 1] / n - pair[j].sum() / n * f1), 5.0 * sig)
    return bad, worst


def compare_draws(ref, actions):
    """The kernel's actions [M, 2] against a ``replay``: (moves differing outside the margin, marks differing
    outside the margin, moves excluded, marks excluded) -- a move is excluded where the row is legal and its move
    margin is <= 1e-5, a mark where its mark margin is <= 1e-6.  A row without a legal move must give move 4 (it
    counts as differing if not)."""
    a = np.asarray(actions).astype(np.int64).reshape(-1, 2)
    mv_ok = ~ref.legal | (ref.move_margin > MOVE_MARGIN)
    mk_ok = ref.mark_margin > MARK_MARGIN
    bad_mv = int((mv_ok & (a[:, 0] != ref.move)).sum())
    bad_mk = int((mk_ok & (a[:, 1] != ref.mark)).sum())
    return bad_mv, bad_mk, int((~mv_ok).sum()), int((~mk_ok).sum())
