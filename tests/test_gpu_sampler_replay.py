"""The action kernels' draws against an independent replay (oracle/sampler.py: Philox4x32-10 from the paper, the
inverse-CDF move and the Bernoulli mark from include/marlmaze.h's description, numpy).

Every kernel that draws goes through act_row: k_act (ops.sample, ops.act), k_head_act (ops.head_act) and the fused
trunk's heads (the rollout at small n).  The inputs, the margins inside which an fp32 kernel may round the other
way and the 0.1 % cap on such rows are oracle.sampler's; tests/test_cpu_sampler_ref.py establishes on the CPU that
the cap and the frequency band hold for the reference on exactly these arrays."""
import numpy as np
import pytest
import torch

from marlmaze import ops
from marlmaze.PPO import PPO
from oracle import sampler as S

pytestmark = pytest.mark.gpu


def _dev(*xs):
    return tuple(torch.as_tensor(x).cuda() for x in xs)


def _host(out):
    a, lp, jl = (x.cpu().numpy() for x in out)
    return a.astype(np.int64), lp, jl


def _run(kernel, ml, kl, mk, seed, offset, offset_dev=None):
    """One launch of `kernel` on the given logits: "sample" / "act" take them as they are, "head" computes them
    from an identity-like head (exactly the same values) at K = 8."""
    if kernel == "head":
        od = None if offset_dev is None else torch.tensor([offset_dev], dtype=torch.int64, device="cuda")
        h, w, b = _dev(*S.identity_head(ml, kl))
        logits = torch.full((ml.shape[0], 6), float("nan"), device="cuda")
        out = ops.head_act(h, w, b, _dev(mk)[0], mode="sample", seed=seed, offset=offset, logits=logits,
                           offset_dev=od)
        assert np.array_equal(logits.cpu().numpy(), np.concatenate([ml, kl.reshape(-1, 1)], 1))
        return _host(out)
    assert offset_dev is None
    dml, dkl, dmk = _dev(ml, kl, mk)
    if kernel == "sample":
        return _host(ops.sample(dml, dkl, dmk, seed, offset))
    return _host(ops.act(dml, dkl, dmk, mode="sample", seed=seed, offset=offset))


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.0, 3.25])
@pytest.mark.parametrize("kernel,M", [("sample", 70001), ("head", 4097)])
def test_exact_inputs_every_row(kernel, M, level):
    """Equal move logits, all legal, mark logit 0: p_j = 1, sum = 5, target = fl(5 u) and sigmoid = 0.5 are exact
    fp32 operations, so the fp32 replay predicts EVERY row -- no margin, no exclusion.  Fails if the uniform is not
    (word >> 8) * 2^-24 (the low bits used, another scale), if output words 0 and 1 are swapped or another word
    feeds a draw, or if the row is not the third counter word.  (< against <=: a row with fl(5 u) on an integer or
    u_mark = 0.5 shows it here too, and test_extreme_uniforms forces the case.)"""
    seed, offset = 2**63 - 25, 2**40 + 7
    ml, kl, mk = S.exact_inputs(M, level)
    ref = S.replay_f32(ml, kl, mk, seed, offset)
    if kernel == "head":  # h = 0 and equal biases: the logits are the biases
        h, w, b = _dev(*S.bias_head(M, [level] * 5, 0.0))
        a, lp, jl = _host(ops.head_act(h, w, b, _dev(mk)[0], mode="sample", seed=seed, offset=offset))
    else:
        a, lp, jl = _run(kernel, ml, kl, mk, seed, offset)
    print(f"{kernel} M={M} level={level}: moves differing {(a[:, 0] != ref.move).sum()}, marks differing "
          f"{(a[:, 1] != ref.mark).sum()}")
    assert np.array_equal(a[:, 0], ref.move)
    assert np.array_equal(a[:, 1], ref.mark)
    np.testing.assert_allclose(lp, np.full(M, np.log(0.2) + np.log(0.5)), rtol=S.RTOL, atol=S.ATOL)


# ---------------------------------------------------------------------------
# b. the general case
# ---------------------------------------------------------------------------
def _check_general(kernel, M, seed, offset, offset_dev=None):
    ml, kl, mk = S.general_inputs(M)
    a, lp, jl = _run(kernel, ml, kl, mk, seed, offset, offset_dev)
    ref = S.replay(ml, kl, mk, seed, offset + (offset_dev or 0))
    bad_mv, bad_mk, ex_mv, ex_mk = S.compare_draws(ref, a)
    print(f"{kernel} M={M} seed={seed:#x} offset={offset:#x} dev={offset_dev}: excluded {ex_mv} (move) + {ex_mk} "
          f"(mark) = {100.0 * (ex_mv + ex_mk) / M:.4f} % of the rows; differing outside the margins: {bad_mv} moves, "
          f"{bad_mk} marks")
    assert bad_mv == 0 and bad_mk == 0
    assert ex_mv + ex_mk <= S.MAX_EXCLUDED * M
    legal = ref.legal
    assert not legal[3] and (a[~legal, 0] == 4).all() and np.isnan(lp[~legal]).all()
    one = mk[:, :5].sum(1) == 1
    assert one[1] and one.sum() > 1 and np.array_equal(a[one, 0], np.argmax(mk[one, :5], 1))
    assert mk[np.arange(M)[legal], a[legal, 0]].all() and (a[mk[:, 5] == 0, 1] == 0).all()
    want = S.logp64(ml, kl, mk, a)  # of the kernel's own action
    err = np.abs(lp[legal] - want[legal])
    print(f"  logp max abs err {err.max():.3g}")
    np.testing.assert_allclose(lp[legal], want[legal], rtol=S.RTOL, atol=S.ATOL)
    lp2 = np.concatenate([lp, np.zeros(M % 2, np.float32)]).reshape(-1, 2)
    assert np.array_equal(jl, (lp2[:, 0] + lp2[:, 1]).astype(np.float32), equal_nan=True)
    return a


@pytest.mark.parametrize("seed,offset,offset_dev", S.GENERAL_CASES)
@pytest.mark.parametrize("kernel,M", [("sample", S.GENERAL_M), ("act", S.GENERAL_M), ("head", 4097)])
def test_general_draws_equal_the_replay(kernel, M, seed, offset, offset_dev):
    """N(0, 2) logits under random masks (and the forced rows: one legal move, mark disallowed, no legal move):
    moves and marks equal the fp64 replay outside the margins, at most 0.1 % of the rows inside them; log-probs
    within rtol 1e-5 / atol 1e-6 of the fp64 log-prob of the kernel's action; joint = the pair's fp32 sum.
    The (seed, offset) pairs have the key's and the counter's high words set, a low word of all ones and a low
    word of zero: the test fails if the key's or the offset's high word is dropped or the two are exchanged."""
    _check_general(kernel, M, seed, offset, offset_dev)


def test_device_base_carries_into_the_high_word():
    """k_head_act with offset 2^32 - 2 and a device base of 5: the draws are those of offset 2^32 + 3 -- fails if
    the base is added to the low word alone (a lost carry) or not at all."""
    seed, offset, base = S.DEVICE_BASE_CASE
    a = _check_general("head", 4097, seed, offset, base)
    ml, kl, mk = S.general_inputs(4097)
    for other in (offset, (offset + base) & 0xFFFFFFFF):  # no base; the carry lost
        r = S.replay(ml, kl, mk, seed, other)
        assert (r.move != a[:, 0]).mean() > 0.2


def test_high_words_of_seed_and_offset_count():
    """Two seeds that share their low word, and two offsets that do, give different actions."""
    ml, kl, mk = S.general_inputs(4097)
    base = _run("sample", ml, kl, mk, 11, 5)[0]
    for kernel in ("sample", "head"):
        for seed, offset in ((11 + 2**32, 5), (11, 5 + 2**32), (11 + 2**63, 5), (11, 5 + 2**63)):
            a = _run(kernel, ml, kl, mk, seed, offset)[0]
            assert (a[:, 0] != base[:, 0]).mean() > 0.2 and (a[:, 1] != base[:, 1]).mean() > 0.1, (kernel, seed, offset)


# ---------------------------------------------------------------------------
# c. extreme uniforms
# ---------------------------------------------------------------------------
EXTREME = [  # edge offset, move logits, mark logit, (move, mark index checked, wanted value)
    ("move_zero", [-200.0, 0, 0, 0, 0], 0.5, 0, 1),
    ("move_max", [0, 0, 0, 0, -200.0], 0.5, 0, 3),
    ("mark_zero", [0.5, -1, 0, 2, 1], -200.0, 1, 0),
    ("mark_max", [0.5, -1, 0, 2, 1], 200.0, 1, 1),
]


@pytest.mark.parametrize("kernel", ["sample", "head"])
@pytest.mark.parametrize("name,move_logits,mark_logit,which,want", EXTREME)
def test_extreme_uniforms(kernel, name, move_logits, mark_logit, which, want):
    """One row at seed 11 and the offset whose draw is u = 0 or u = 1 - 2^-24 (oracle.sampler.EDGE_OFFSETS).
    u_move = 0 against a first move whose exp underflows to 0: 0 < 0 is false, the move is 1 -- it is 0 if the
    comparison is <=.  u_move = 1 - 2^-24 against a last move of weight 0: the move is 3, never 4 (a draw that
    walks past the end, or <=, takes 4).  u_mark = 0 at sigmoid = 0: no mark (<= marks).  u_mark = 1 - 2^-24 at
    sigmoid = 1: the mark.  Every log-prob is finite and within the bar of the fp64 one."""
    offset = S.EDGE_OFFSETS[name][0]
    ml = np.float32([move_logits])
    kl = np.float32([mark_logit])
    mk = np.ones((1, 6), np.uint8)
    if kernel == "head":
        h, w, b = _dev(*S.bias_head(1, move_logits, mark_logit))
        a, lp, jl = _host(ops.head_act(h, w, b, _dev(mk)[0], mode="sample", seed=S.EDGE_SEED, offset=offset))
    else:
        a, lp, jl = _run(kernel, ml, kl, mk, S.EDGE_SEED, offset)
    print(f"{kernel} {name}: action {a[0].tolist()} logp {lp[0]!r}")
    assert a[0, which] == want
    ref = S.replay(ml, kl, mk, S.EDGE_SEED, offset)  # the other draw is an ordinary one: as replayed
    assert min(ref.move_margin[0], ref.mark_margin[0]) < 1e-7 < max(ref.move_margin[0], ref.mark_margin[0])
    assert a[0, 1 - which] == (ref.mark[0], ref.move[0])[which]
    want_lp = S.logp64(ml, kl, mk, a)
    assert np.isfinite(lp).all() and np.isfinite(jl).all()
    np.testing.assert_allclose(lp, want_lp, rtol=S.RTOL, atol=S.ATOL)
    assert jl[0] == lp[0]


# ---------------------------------------------------------------------------
# d. frequencies
# ---------------------------------------------------------------------------
def test_frequencies_of_64_distributions():
    """64 distributions (one, two, five legal moves; mark logits in [-3, 3]; the mark disallowed), 8,192 rows
    each, one launch of 524,288 rows.  Per class and cell (five moves, the mark): the frequency within
    5 sqrt(p (1 - p) / n) + 1 / n of the fp64 probability; the probability the stored log-probs state within the
    same bound of the frequency (>= 100 draws); move and mark independent within 5 sigma
    (oracle.sampler.frequency_report).  Fails if the draw does not follow the distribution whose log-prob is
    stored, or if both draws come from one output word."""
    classes, (ml, kl, mk) = S.freq_inputs()
    a, lp, _ = _run("sample", ml, kl, mk, S.FREQ_SEED, S.FREQ_OFFSET)
    bad, worst = S.frequency_report(classes, a, lp)
    print("worst |deviation| / bound: freq %.3f, stored %.3f, independence %.3f" % tuple(worst))
    assert not bad, bad


# ---------------------------------------------------------------------------
# e. the rollout's counters
# ---------------------------------------------------------------------------
def test_rollout_draws_are_seed_offset_row():
    """Eager and captured rollouts (n = 512, T = 8, three each): step t's stored actions are the replay of
    (sample_seed, offset before the rollout + t, row) on the step's stored masks and the actor's logits of the
    stored observations (Actor.logits: bit-equal to the rollout's).  Fails if a step reuses an offset, if the
    rollouts do not continue each other's offsets, or if a graph replay's device base did not advance (the third
    captured rollout is a replay); the seed's high word is set."""
    cfg = dict(default_size=(6, 6), max_timestep=20, seed_base=7)
    n, T = 512, 8
    for graph in (False, True):
        ag = PPO(2, load=False, verbose=False, save=False, n_envs=n, horizon=T, batch_size=n * T,
                 sample_seed=2**62 + 5, env_config=cfg, graph_rollout=graph)
        with torch.no_grad():  # non-trivial policies (the 0.01 init makes every logit ~0)
            ag.actor.move_head.weight.mul_(30.0)
            ag.actor.mark_head.weight.mul_(30.0)
        assert ag.sample_seed == 2**62 + 5
        for it in range(3):
            off0 = ag._sample_offset
            b = ag.rollout()
            assert ag._sample_offset == off0 + T
            bad_mv = bad_mk = excluded = 0
            for t in range(T):
                with torch.no_grad():
                    z = ag.actor.logits(b["obs"][t].view(2 * n, 65)).cpu().numpy()
                mk = b["masks"][t].view(2 * n, 6).cpu().numpy()
                a = b["act"][t].view(2 * n, 2).cpu().numpy()
                ref = S.replay(z[:, :5], z[:, 5], mk, ag.sample_seed, off0 + t)
                mv, km, ex_mv, ex_mk = S.compare_draws(ref, a)
                bad_mv, bad_mk, excluded = bad_mv + mv, bad_mk + km, excluded + ex_mv + ex_mk
                # the draws are not trivial: the next step's offset does not fit this step (ten rows of the
                # 1,024 are ten times what exposes a reused offset)
                other = S.replay(z[:, :5], z[:, 5], mk, ag.sample_seed, off0 + t + 1)
                assert (other.move != a[:, 0]).sum() + (other.mark != a[:, 1]).sum() >= 10
                np.testing.assert_allclose(b["rowlogp"][t].cpu().numpy()[ref.legal],
                                           S.logp64(z[:, :5], z[:, 5], mk, a)[ref.legal], rtol=S.RTOL, atol=S.ATOL)
            print(f"graph={graph} rollout {it} (offset {off0}): excluded {excluded} of {T * 2 * n} rows "
                  f"({100.0 * excluded / (T * 2 * n):.4f} %), differing {bad_mv} moves {bad_mk} marks")
            assert bad_mv == 0 and bad_mk == 0
            assert excluded <= S.MAX_EXCLUDED * T * 2 * n
            ag._carry_over()
        if graph:
            assert ag._graph is not None
