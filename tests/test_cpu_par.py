"""The par constants of include/marlmaze.h and their mirrors in marlmaze._lib are the same numbers, and the host
side of the par evaluation (result_from_par_words, format_result) turns words into the documented keys."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "marlmaze.h")

SCALARS = ["MM_PAR_EPISODES", "MM_PAR_SUM_LEN", "MM_PAR_SUM_PAR", "MM_PAR_SUM_RATIO_Q16", "MM_PAR_AT_PAR",
           "MM_PAR_BELOW", "MM_PAR_UNRATED", "MM_PAR_MAX_EXCESS"]


def _defines():
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(MM_PAR_\w+)\s+(\d+)\b", text, re.M)}


def test_par_constants_equal_their_python_mirrors():
    from marlmaze import _lib

    d = _defines()
    names = ["MM_PAR_WORDS"] + SCALARS + ["MM_PAR_HIST0", "MM_PAR_HIST_BINS"]
    assert sorted(d) == sorted(names)  # every MM_PAR_* of the header has a mirror
    for name in names:
        assert getattr(_lib, name[3:]) == d[name], name
    scalars = [d[n] for n in SCALARS]
    assert len(set(scalars)) == len(SCALARS) and max(scalars) < d["MM_PAR_HIST0"]
    assert d["MM_PAR_HIST0"] + d["MM_PAR_HIST_BINS"] == d["MM_PAR_WORDS"] == 32
    for sym in ("mm_env_dist", "mm_env_par", "mm_par_init", "mm_par_accum"):
        assert sym in _lib.EXPORTS


def test_result_from_par_words():
    from marlmaze import _lib
    from marlmaze.evaluate import PAR_BIN_EDGES, result_from_par_words

    r = result_from_par_words([0] * _lib.PAR_WORDS)
    assert r["par_episodes"] == 0 and r["mean_par"] is None and r["mean_par_ratio"] is None
    assert r["at_par"] == r["below_par"] == r["par_unrated"] == r["max_excess"] == 0
    assert r["par_hist"] == [0] * 16 and r["par_bin_edges"] == PAR_BIN_EDGES
    assert PAR_BIN_EDGES[0] == 1.0 and PAR_BIN_EDGES[1] == 1.25 and PAR_BIN_EDGES[-1] == 4.75

    # three rated episodes: (len, par) = (10, 10), (15, 10), (70, 10); one unrated
    w = [0] * _lib.PAR_WORDS
    pairs = [(10, 10), (15, 10), (70, 10)]
    w[_lib.PAR_EPISODES] = 3
    w[_lib.PAR_SUM_LEN] = sum(a for a, _ in pairs)
    w[_lib.PAR_SUM_PAR] = sum(p for _, p in pairs)
    w[_lib.PAR_SUM_RATIO_Q16] = sum(a * 65536 // p for a, p in pairs)
    w[_lib.PAR_AT_PAR] = 1
    w[_lib.PAR_UNRATED] = 1
    w[_lib.PAR_MAX_EXCESS] = 60
    for a, p in pairs:
        w[_lib.PAR_HIST0 + min(max(4 * a // p - 4, 0), 15)] += 1
    r = result_from_par_words(w)
    assert set(r) == {"par_episodes", "mean_par", "mean_par_ratio", "at_par", "below_par", "par_unrated", "max_excess",
                      "par_hist", "par_bin_edges"}
    assert r["par_episodes"] == 3 and r["mean_par"] == 10.0 and r["at_par"] == 1 and r["below_par"] == 0
    assert r["par_unrated"] == 1 and r["max_excess"] == 60
    assert abs(r["mean_par_ratio"] - (1.0 + 1.5 + 7.0) / 3) < 1e-12  # every ratio here is exact in Q16
    assert r["par_hist"] == [1, 0, 1] + [0] * 12 + [1]


def test_format_result_with_and_without_par():
    from marlmaze import _lib
    from marlmaze.evaluate import format_result, result_from_par_words, result_from_words

    w = [0] * _lib.EVAL_WORDS
    w[_lib.EV_EPISODES], w[_lib.EV_SOLVED], w[_lib.EV_SUM_LEN], w[_lib.EV_SUM_LEN_SOLVED] = 2, 2, 50, 50
    w[_lib.EV_SUM_SHORT_SOLVED], w[_lib.EV_SUM_RATIO_Q16] = 20, 5 * 65536
    w[_lib.EV_MIN_LEN_SOLVED], w[_lib.EV_MAX_LEN_SOLVED] = 20, 30
    base = result_from_words(w)
    plain = format_result(base)
    assert "par" not in plain
    pw = [0] * _lib.PAR_WORDS
    pw[_lib.PAR_EPISODES], pw[_lib.PAR_SUM_LEN], pw[_lib.PAR_SUM_PAR] = 2, 50, 40
    pw[_lib.PAR_SUM_RATIO_Q16], pw[_lib.PAR_AT_PAR] = 65536 + 65536 * 3 // 2, 1
    both = format_result({**base, **result_from_par_words(pw)})
    assert both.startswith(plain) and both[len(plain):] == "; vs par 20.00 (ratio 1.250, 1 at par)"
    # no rated episode: the means are None and print as "-"
    none = format_result({**base, **result_from_par_words([0] * _lib.PAR_WORDS)})
    assert none.endswith("; vs par - (ratio -, 0 at par)")
    timed = format_result({**base, **result_from_par_words(pw), "env_steps": 100, "seconds": 2.0})
    assert "at par); 100 env-steps in 2.00 s" in timed
