"""oracle/sampler.py, the sampler's independent reference, checked without a GPU: Philox4x32-10 against the
Random123 known answers, the replay against the actions a real GPU recorded (tests/golden/sampler_pinned.npz), the
four extreme-uniform counters, and the conditions under which tests/test_gpu_sampler_replay.py's bounds are valid
(few rows near a decision boundary; the reference's own frequencies inside the 5 sigma band), on exactly the
arrays the GPU tests use."""
import numpy as np
import pytest

from oracle import sampler as S

# tests/test_gpu_eval.py's SHAPES without the shape the fixture holds as digests only
SHAPES = [(M, K) for M in (1, 2, 31, 33, 4097) for K in (8, 264) if (M, K) != (4097, 264)]


def _hex(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("ctr,key,out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    """Random123's kat_vectors for philox4x32-10."""
    assert S.philox4x32_10(_hex(ctr), _hex(key)).tolist() == _hex(out)


def test_philox_is_vectorised():
    """An array of counters gives each counter's own answer, and `words` places (offset, row) and the seed."""
    c = np.array([_hex("0 0 0 0"), _hex("243f6a88 85a308d3 13198a2e 03707344")], np.uint64)
    k = np.array([_hex("0 0"), _hex("a4093822 299f31d0")], np.uint64)
    assert S.philox4x32_10(c, k).tolist() == [_hex("6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                                              _hex("d16cfe09 94fdcceb 5001e420 24126ea1")]
    w = S.words(0x299F31D0A4093822, 0x85A308D3243F6A88, [0x13198A2E])
    assert w.tolist() == [S.philox4x32_10(_hex("243f6a88 85a308d3 13198a2e 0"), _hex("a4093822 299f31d0")).tolist()]
    assert S.words(0, 0, 3)[0].tolist() == _hex("6627e8d5 e169c58d bc57ac4c 9b00dbd8")


@pytest.mark.parametrize("tag,offset", [("s", 5), ("hs", 5), ("hsd", 5 + 3)])
@pytest.mark.parametrize("M,K", SHAPES)
def test_replay_gives_the_recorded_actions(golden, M, K, tag, offset):
    """The fp64 replay of the recorded logits and masks at seed 11 gives the actions an MI355X recorded (offset 5;
    5 plus the device base 3 for hsd), outside the margins; the recorded log-probs are within the sampler's bar of
    the replay's fp64 ones; the row without a legal move gives move 4 and NaN."""
    fx = golden("sampler_pinned")
    lg, mk = fx[f"{M}x{K}/hs_logits"], fx[f"{M}x{K}/mk"]
    a, lp = fx[f"{M}x{K}/{tag}_a"], fx[f"{M}x{K}/{tag}_lp"]
    r = S.replay(lg[:, :5], lg[:, 5], mk, 11, offset)
    bad_mv, bad_mk, ex_mv, ex_mk = S.compare_draws(r, a)
    print(f"{M}x{K} {tag}: rows excluded {ex_mv} (move) {ex_mk} (mark) of {M}")
    assert bad_mv == 0 and bad_mk == 0
    assert ex_mv + ex_mk <= 1
    assert np.array_equal(r.legal, mk[:, :5].any(1))
    if M > 2:
        assert not r.legal[3] and (~r.legal).sum() >= 1
    assert (a[~r.legal, 0] == 4).all() and (r.move[~r.legal] == 4).all()
    assert np.isnan(lp[~r.legal]).all() and np.isnan(r.logp[~r.legal]).all()
    # the recorded log-prob is that of the recorded action
    ref = S.logp64(lg[:, :5], lg[:, 5], mk, a)
    np.testing.assert_allclose(lp[r.legal], ref[r.legal], rtol=S.RTOL, atol=S.ATOL)
    same = r.legal & (a[:, 0] == r.move) & (a[:, 1] == r.mark)
    assert np.array_equal(ref[same], r.logp[same])


@pytest.mark.parametrize("name", sorted(S.EDGE_OFFSETS))
def test_edge_counters(name):
    """The offsets whose row-0 draw at seed 11 is an extreme uniform: the output word and the uniform."""
    offset, word, value, u = S.EDGE_OFFSETS[name]
    assert int(S.words(S.EDGE_SEED, offset, 1)[0, word]) == value
    assert float(S.uniforms(S.EDGE_SEED, offset, 1)[word][0]) == u
    assert u in (0.0, 1 - 2.0**-24)


def test_uniforms_are_exact_fp32():
    um, uk = S.uniforms(2**63 - 25, 2**40 + 7, 4096)
    for u in (um, uk):
        assert (u >= 0).all() and (u <= 1 - 2.0**-24).all()
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and np.array_equal(u * 2.0**24 % 1, 0 * u)


def test_exact_inputs_f32_equals_f64():
    """On the exact inputs (equal logits, mark logit 0) the fp32 and the fp64 replay differ at most where fl(5 u)
    rounds onto a cumulative sum: the fp32 one is the kernel's prediction, and the two agree almost everywhere."""
    for level in (0.0, 3.25):
        ml, kl, mk = S.exact_inputs(S.GENERAL_M, level)
        r32, r64 = S.replay_f32(ml, kl, mk, 11, 5), S.replay(ml, kl, mk, 11, 5)
        assert np.array_equal(r32.mark, r64.mark)  # u < 0.5 has no rounding
        diff = r32.move != r64.move
        assert diff.sum() <= 5 and (r64.move_margin[diff] < 2.0**-23).all()
        assert set(np.unique(r32.move)) == {0, 1, 2, 3, 4} and set(np.unique(r32.mark)) == {0, 1}


@pytest.mark.parametrize("seed,offset", [(s, o) for s, o, _ in S.GENERAL_CASES]
                         + [(S.DEVICE_BASE_CASE[0], S.DEVICE_BASE_CASE[1] + S.DEVICE_BASE_CASE[2])])
@pytest.mark.parametrize("M", [S.GENERAL_M, 4097])
def test_general_inputs_have_few_rows_near_a_boundary(M, seed, offset):
    """The exclusion cap of the GPU test holds on the reference: at most 0.1 % of the rows are within the margins
    (and for 70,001 rows the forced rows are there)."""
    ml, kl, mk = S.general_inputs(M)
    r = S.replay(ml, kl, mk, seed, offset)
    ex_mv = int((r.legal & (r.move_margin <= S.MOVE_MARGIN)).sum())
    ex_mk = int((r.mark_margin <= S.MARK_MARGIN).sum())
    print(f"M={M} seed={seed:#x} offset={offset:#x}: excluded {ex_mv} (move) {ex_mk} (mark)")
    assert ex_mv + ex_mk <= S.MAX_EXCLUDED * M
    assert mk[1, :5].sum() == 1 and r.move[1] == 2 and not mk[2, 5] and r.mark[2] == 0
    assert not r.legal[3] and r.move[3] == 4 and np.isnan(r.logp[3]) and r.legal.sum() >= M - 1 - 0.02 * M


def test_high_words_change_the_draws():
    """Seeds (offsets) that share their low word draw differently: the GPU test's assertion is satisfiable."""
    ml, kl, mk = S.general_inputs(4097)
    base = S.replay(ml, kl, mk, 11, 5)
    for seed, offset in ((11 + 2**32, 5), (11, 5 + 2**32)):
        r = S.replay(ml, kl, mk, seed, offset)
        assert (r.move != base.move).mean() > 0.2 and (r.mark != base.mark).mean() > 0.1


def test_frequency_inputs_pass_on_the_reference():
    """The 5 sigma band of the GPU frequency test holds for the reference's own draws on the same 64 classes at
    the same (seed, offset) -- the first pair tried -- and the classes are the ones asked for."""
    classes, rows = S.freq_inputs()
    ml, kl, mk = classes
    nlegal = mk[:, :5].sum(1)
    assert {1, 2, 5} <= set(nlegal.tolist()) and nlegal.min() >= 1
    assert (np.abs(kl) <= 3).all() and kl.min() < -2 and kl.max() > 2 and 0 < mk[:, 5].sum() < len(kl)
    r = S.replay(*rows, S.FREQ_SEED, S.FREQ_OFFSET)
    assert int((r.move_margin <= S.MOVE_MARGIN).sum() + (r.mark_margin <= S.MARK_MARGIN).sum()) \
        <= S.MAX_EXCLUDED * len(r.move)
    bad, worst = S.frequency_report(classes, np.stack([r.move, r.mark], 1), r.logp)
    print("worst |deviation| / bound: freq %.3f, stored %.3f, independence %.3f" % tuple(worst))
    assert not bad, bad
    # the check bites: a sampler that ignored the mask's mark byte, or shifted one class's moves, is caught
    a = np.stack([r.move, r.mark], 1)
    shifted = a.copy()
    shifted[4 * S.FREQ_ROWS:5 * S.FREQ_ROWS, 0] = (shifted[4 * S.FREQ_ROWS:5 * S.FREQ_ROWS, 0] + 1) % 5
    assert S.frequency_report(classes, shifted, r.logp)[0]
    tied = a.copy()
    pm = S.probs64(*rows)[1]  # the mark drawn from the move's uniform: the right frequency, not independent
    tied[:, 1] = S.uniforms(S.FREQ_SEED, S.FREQ_OFFSET, len(a))[0] < pm
    bad = S.frequency_report(classes, tied, r.logp)[0]
    assert bad and all(" x mark" in b or "stored" in b for b in bad), bad
