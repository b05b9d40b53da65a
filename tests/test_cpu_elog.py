"""The episode-log constants of include/marlmaze.h and their mirrors in marlmaze._lib are the same numbers, the
library exports the four entry points, and the host side (behaviour_sums, behaviour_from_sums, worst_records,
format_result) turns records into the documented statistics."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "marlmaze.h")

WORDS = ["MM_ELOG_LEN", "MM_ELOG_SHORTEST", "MM_ELOG_SOLVED", "MM_ELOG_PAR", "MM_ELOG_T_KEY", "MM_ELOG_FETCHER",
         "MM_ELOG_T_KNOW0", "MM_ELOG_T_KNOW1", "MM_ELOG_T_READY", "MM_ELOG_CELLS0", "MM_ELOG_CELLS1",
         "MM_ELOG_CELLS_BOTH", "MM_ELOG_OPEN", "MM_ELOG_MARKS0", "MM_ELOG_MARKS1", "MM_ELOG_STAYS"]
SYMBOLS = ("mm_elog_state_words", "mm_elog_init", "mm_elog_start", "mm_elog_step")


def _defines():
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(MM_ELOG_\w+)\s+(\d+)\b", text, re.M)}


def test_elog_constants_equal_their_python_mirrors():
    from marlmaze import _lib

    d = _defines()
    assert sorted(d) == sorted(["MM_ELOG_WORDS"] + WORDS)  # every MM_ELOG_* of the header has a mirror
    for name in d:
        assert getattr(_lib, name[3:]) == d[name], name
    assert d["MM_ELOG_WORDS"] == 16
    assert sorted(d[w] for w in WORDS) == list(range(16))  # distinct, in 0..15
    # the table of the record, word by word, and the field names in the same order
    assert [d[w] for w in WORDS] == list(range(16))
    assert list(_lib.ELOG_FIELDS) == [w[len("MM_ELOG_"):] for w in WORDS]
    assert _lib.VERSION == 308


def test_library_exports_the_elog_symbols():
    from marlmaze import _build, _lib

    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and getattr(L, sym) is not None
        assert re.search(rf"\bT {sym}\b", nm), sym
    # two bitmaps of ceil(stride / 32) words plus the scalars: the scalars are what is left at any stride
    words = {s: L.mm_elog_state_words(s) for s in (1, 32, 33, 49, 361, 1681)}
    scalars = words[1] - 2
    assert 9 <= scalars <= 16
    for s, v in words.items():
        assert v == scalars + 2 * ((s + 31) // 32), s
    assert L.mm_elog_state_words(0) < 0
    # host-side argument checks (nothing is launched): null buffers, a misaligned log, a wrong state size
    assert L.mm_elog_init(None, None, None, 4, 1, words[49], None) == _lib_e_arg()
    assert L.mm_elog_init(8, 16, 32, 4, 1, words[49], None) == _lib_e_arg()  # log not 16-byte aligned
    assert L.mm_elog_start(None, None, None, words[49], None) != 0
    assert L.mm_elog_step(None, None, None, None, None, None, 1, None, None, words[49], None, None) != 0


def _lib_e_arg():
    return int(re.search(r"#define MM_E_ARG \((-\d+)\)", open(HEADER).read()).group(1))


def _records(rows):
    from marlmaze.evaluate import RECORD_DTYPE

    out = np.zeros(len(rows), RECORD_DTYPE)
    for i, row in enumerate(rows):
        for k, v in row.items():
            out[i][k] = v
    return out


# three hand-made episodes: solved by agent 1 fetching; timed out with the key found by agent 0, never exit-ready;
# timed out without the key
ROWS = [dict(maze=0, episode=0, LEN=30, SHORTEST=6, SOLVED=1, PAR=12, T_KEY=10, FETCHER=1, T_KNOW0=0, T_KNOW1=14,
             T_READY=20, CELLS0=9, CELLS1=7, CELLS_BOTH=4, OPEN=24, MARKS0=3, MARKS1=1, STAYS=2),
        dict(maze=1, episode=0, LEN=40, SHORTEST=8, SOLVED=0, PAR=15, T_KEY=30, FETCHER=0, T_KNOW0=-1, T_KNOW1=5,
             T_READY=-1, CELLS0=10, CELLS1=6, CELLS_BOTH=0, OPEN=24, MARKS0=0, MARKS1=2, STAYS=0),
        dict(maze=1, episode=1, LEN=40, SHORTEST=4, SOLVED=0, PAR=-1, T_KEY=-1, FETCHER=-1, T_KNOW0=-1, T_KNOW1=-1,
             T_READY=-1, CELLS0=5, CELLS1=5, CELLS_BOTH=5, OPEN=22, MARKS0=0, MARKS1=0, STAYS=7)]


def test_behaviour_from_sums_on_hand_made_records():
    from marlmaze.evaluate import BEHAVIOUR_SUMS, behaviour_from_sums, behaviour_sums

    s = behaviour_sums(_records(ROWS))
    assert list(s) == list(BEHAVIOUR_SUMS) and all(type(v) is int for v in s.values())
    assert s == dict(episodes=3, key_found=2, sum_t_key=40, ready=1, sum_t_ready=20, solved_ready=1, sum_t_exit=10,
                     sum_covered=12 + 16 + 5, sum_both=9, sum_open=70, fetched=2, fetched_by_0=1, sum_marks=6,
                     sum_stays=9)
    b = behaviour_from_sums(s)
    assert set(b) == {"key_found_rate", "mean_t_key", "mean_t_ready", "mean_t_exit", "coverage", "overlap",
                      "fetcher_share", "marks_per_episode", "stays_per_episode"}
    assert b["key_found_rate"] == 2 / 3 and b["mean_t_key"] == 20.0 and b["mean_t_ready"] == 20.0
    assert b["mean_t_exit"] == 10.0 and b["coverage"] == 33 / 70 and b["overlap"] == 9 / 33
    assert b["fetcher_share"] == 0.5 and b["marks_per_episode"] == 2.0 and b["stays_per_episode"] == 3.0
    # a summed vector in BEHAVIOUR_SUMS order (what DP ranks add up) gives the same, and two ranks' sums add
    assert behaviour_from_sums([s[k] for k in BEHAVIOUR_SUMS]) == b
    assert behaviour_from_sums([2 * s[k] for k in BEHAVIOUR_SUMS]) == b
    with pytest.raises(ValueError):
        behaviour_from_sums([1, 2, 3])


def test_behaviour_of_nothing_is_none():
    from marlmaze.evaluate import behaviour_from_sums, behaviour_sums

    s = behaviour_sums(_records([]))
    assert all(v == 0 for v in s.values())
    assert all(v is None for v in behaviour_from_sums(s).values())
    # episodes without a key, a ready team or a pickup: those means are None, the per-episode ones are numbers
    b = behaviour_from_sums(behaviour_sums(_records(ROWS[2:])))
    assert b["key_found_rate"] == 0.0 and b["mean_t_key"] is None and b["mean_t_ready"] is None
    assert b["mean_t_exit"] is None and b["fetcher_share"] is None
    assert b["coverage"] == 5 / 22 and b["overlap"] == 1.0 and b["stays_per_episode"] == 7.0


def test_worst_records_and_the_result_line():
    from marlmaze import _lib
    from marlmaze.evaluate import behaviour_from_sums, behaviour_sums, format_result, result_from_words, worst_records

    r = _records(ROWS)
    assert [int(x["LEN"] - max(x["PAR"], 0)) for x in worst_records(r, 2, True)] == [40, 25]  # the unrated one first
    assert [(int(x["maze"]), int(x["episode"])) for x in worst_records(r, 5, False)] == [(1, 0), (1, 1), (0, 0)]
    assert len(worst_records(r, 0, False)) == 0
    base = result_from_words([0] * _lib.EVAL_WORDS)
    plain = format_result(base)
    both = format_result({**base, "behaviour": behaviour_from_sums(behaviour_sums(r))})
    assert both.startswith(plain) and both[len(plain):] == ("; key found in 0.6667 at t 20.00, exit-ready at t 20.00, "
                                                            "out in 10.00, coverage 0.471 (overlap 0.273)")
    none = format_result({**base, "behaviour": behaviour_from_sums(behaviour_sums(_records([])))})
    assert none.endswith("; key found in - at t -, exit-ready at t -, out in -, coverage - (overlap -)")
