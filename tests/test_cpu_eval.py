"""The evaluation constants of include/marlmaze.h and their mirrors in marlmaze._lib are the same numbers."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "marlmaze.h")


def _defines():
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(MM_(?:ACT|EVAL|EV)_\w+)\s+(\d+)\b", text, re.M)}


def test_header_constants_equal_their_python_mirrors():
    from marlmaze import _lib

    d = _defines()
    names = ["MM_ACT_SAMPLE", "MM_ACT_GREEDY", "MM_EVAL_WORDS", "MM_EV_EPISODES", "MM_EV_SOLVED", "MM_EV_TIMEOUTS",
             "MM_EV_SUM_LEN", "MM_EV_SUM_LEN_SOLVED", "MM_EV_SUM_SHORT_SOLVED", "MM_EV_MIN_LEN_SOLVED",
             "MM_EV_MAX_LEN_SOLVED", "MM_EV_SUM_RATIO_Q16", "MM_EV_BAD_SHORT", "MM_EV_HIST0", "MM_EV_HIST_BINS"]
    assert sorted(d) == sorted(names)  # every MM_ACT_* / MM_EVAL_* / MM_EV_* of the header has a mirror
    for name in names:
        assert getattr(_lib, name[3:]) == d[name], name
    assert _lib.ACT_MODES == {"sample": d["MM_ACT_SAMPLE"], "greedy": d["MM_ACT_GREEDY"]}
    # the layout: ten scalar words, distinct, below the histogram, which fills the rest
    scalars = [d[n] for n in names[3:13]]
    assert len(set(scalars)) == 10 and max(scalars) < d["MM_EV_HIST0"]
    assert d["MM_EV_HIST0"] + d["MM_EV_HIST_BINS"] == d["MM_EVAL_WORDS"] == 32


def test_version_is_308():
    from marlmaze import _lib

    assert _lib.VERSION == 308
    for sym in ("mm_head_act", "mm_act", "mm_eval_init", "mm_eval_accum"):
        assert sym in _lib.EXPORTS
