"""Policy evaluation: whole episodes on many mazes at once, counted on the device.

``EvalTotals`` wraps the device buffers of mm_eval_init / mm_eval_accum (csrc/eval_kernels.hip): after every
env step, every maze that finished an episode -- and has not yet contributed its quota of episodes -- adds it
to 32 integer words (episodes, solved, timeouts, sums of lengths and shortest paths, min / max, a histogram of
exit time over shortest path).  Every maze contributes its FIRST ``quota`` episodes and nothing else, so the
result is a per-maze average: without the quota, mazes with short episodes would finish more of them inside
any fixed number of steps and bias the success rate upwards.

``ParTotals`` is its counterpart against par (mm_par_init / mm_par_accum, csrc/solve_kernels.hip): the exit time of
every counted solved episode over the par time of its maze, the length of the shortest possible solving episode
(VecMaze.par).  The floor of that ratio is 1.0, which the ratio over the shortest start -> end path cannot reach:
the key never lies on that path.

``EpisodeLog`` keeps what the totals cannot say: one record per counted episode (mm_elog_init / mm_elog_start /
mm_elog_step, csrc/elog_kernels.hip) -- which maze, its outcome and par, when the key was found and by whom, when
each agent learnt the exit, when the team became exit-ready, the cells each agent covered, its marks and stays.
``behaviour_sums`` / ``behaviour_from_sums`` reduce the records to statistics, each a ratio of two integer sums.

``PPO.evaluate`` drives all three; ``python -m marlmaze.evaluate --model PPO.pth ...`` is the command line.
"""
import argparse
import ctypes
import json
import sys

import numpy as np
import torch

from . import _lib

NONE_MIN = 2**64 - 1  # the min word before any solved episode
RATIO_BIN_EDGES = [1.0 + 0.25 * k for k in range(_lib.EV_HIST_BINS)]  # lower edges; the last bin is open


def result_from_words(words):
    """The 32 uint64 words of a run's totals (python ints) -> the result dict.  Means over nothing are None."""
    w = [int(x) for x in words]
    episodes, solved = w[_lib.EV_EPISODES], w[_lib.EV_SOLVED]
    bad = w[_lib.EV_BAD_SHORT]
    rated = solved - bad  # solved episodes with a shortest path > 0: the ratio's and the histogram's
    div = lambda a, b: (a / b if b else None)  # noqa: E731
    return dict(
        episodes=episodes, solved=solved, timeouts=w[_lib.EV_TIMEOUTS], success_rate=div(solved, episodes),
        mean_len=div(w[_lib.EV_SUM_LEN], episodes), mean_len_solved=div(w[_lib.EV_SUM_LEN_SOLVED], solved),
        mean_shortest_solved=div(w[_lib.EV_SUM_SHORT_SOLVED], solved),
        mean_ratio=div(w[_lib.EV_SUM_RATIO_Q16] / 65536.0, rated),
        min_len_solved=(w[_lib.EV_MIN_LEN_SOLVED] if solved else None),
        max_len_solved=(w[_lib.EV_MAX_LEN_SOLVED] if solved else None),
        ratio_hist=w[_lib.EV_HIST0:_lib.EV_HIST0 + _lib.EV_HIST_BINS], ratio_bin_edges=list(RATIO_BIN_EDGES),
        bad_shortest=bad)


PAR_BIN_EDGES = [1.0 + 0.25 * k for k in range(_lib.PAR_HIST_BINS)]  # lower edges; the last bin is open


def result_from_par_words(words):
    """The 32 uint64 words of a run's totals against par (python ints) -> the par keys of the result dict.
    Means over nothing are None."""
    w = [int(x) for x in words]
    rated = w[_lib.PAR_EPISODES]
    div = lambda a, b: (a / b if b else None)  # noqa: E731
    return dict(
        par_episodes=rated, mean_par=div(w[_lib.PAR_SUM_PAR], rated),
        mean_par_ratio=div(w[_lib.PAR_SUM_RATIO_Q16] / 65536.0, rated), at_par=w[_lib.PAR_AT_PAR],
        below_par=w[_lib.PAR_BELOW], par_unrated=w[_lib.PAR_UNRATED], max_excess=w[_lib.PAR_MAX_EXCESS],
        par_hist=w[_lib.PAR_HIST0:_lib.PAR_HIST0 + _lib.PAR_HIST_BINS], par_bin_edges=list(PAR_BIN_EDGES))


class EvalTotals:
    """Device totals of an evaluation over ``n`` mazes, ``quota`` episodes per maze.

    init() and accum() are stream-ordered launches (no allocation, no synchronisation); words() and read()
    copy the 32 words to the host."""

    def __init__(self, n, quota=1, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.quota = int(n), int(quota)
        self.totals = torch.empty(_lib.EVAL_WORDS, dtype=torch.int64, device=device)  # uint64 words
        self.counted = torch.empty(self.n, dtype=torch.int32, device=device)
        self.init()

    def init(self):
        _lib.check(_lib.lib().mm_eval_init(_lib.ptr(self.totals), _lib.ptr(self.counted), self.n, _lib.stream_ptr()),
                   "mm_eval_init")

    def accum(self, done, reward, ep_stats):
        """One env step's done [n] u8, reward [n] f32 and ep_stats [n, 2] int32 (VecMaze.step's)."""
        if (done.dtype != torch.uint8 or reward.dtype != torch.float32 or ep_stats.dtype != torch.int32
                or done.numel() != self.n or reward.numel() != self.n or ep_stats.numel() != 2 * self.n
                or not (done.is_contiguous() and reward.is_contiguous() and ep_stats.is_contiguous())):
            raise ValueError("EvalTotals.accum: done [n] uint8, reward [n] float32, ep_stats [n, 2] int32, contiguous")
        _lib.check(_lib.lib().mm_eval_accum(_lib.ptr(done), _lib.ptr(reward), _lib.ptr(ep_stats), self.n, self.quota,
                                            _lib.ptr(self.counted), _lib.ptr(self.totals), _lib.stream_ptr()),
                   "mm_eval_accum")

    def words(self):
        """The 32 words as python ints (uint64).  Synchronises."""
        return [int(v) & (2**64 - 1) for v in self.totals.tolist()]

    def read(self):
        return result_from_words(self.words())


class ParTotals:
    """Device totals of exit time against par over ``n`` mazes, ``quota`` episodes per maze (EvalTotals' shape,
    with a ``counted`` array of its own).

    init() and accum() are stream-ordered launches (no allocation, no synchronisation); words() and read()
    copy the 32 words to the host."""

    def __init__(self, n, quota=1, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.quota = int(n), int(quota)
        self.totals = torch.empty(_lib.PAR_WORDS, dtype=torch.int64, device=device)  # uint64 words
        self.counted = torch.empty(self.n, dtype=torch.int32, device=device)
        self.init()

    def init(self):
        _lib.check(_lib.lib().mm_par_init(_lib.ptr(self.totals), _lib.ptr(self.counted), self.n, _lib.stream_ptr()),
                   "mm_par_init")

    def accum(self, done, reward, ep_stats, par):
        """One env step's done [n] u8, reward [n] f32 and ep_stats [n, 2] int32 (VecMaze.step's), and the par
        rows [n, 4] int32 (VecMaze.par's) of the mazes that were stepped."""
        if (done.dtype != torch.uint8 or reward.dtype != torch.float32 or ep_stats.dtype != torch.int32
                or par.dtype != torch.int32 or done.numel() != self.n or reward.numel() != self.n
                or ep_stats.numel() != 2 * self.n or par.numel() != 4 * self.n
                or not (done.is_contiguous() and reward.is_contiguous() and ep_stats.is_contiguous()
                        and par.is_contiguous())):
            raise ValueError("ParTotals.accum: done [n] uint8, reward [n] float32, ep_stats [n, 2] int32, "
                             "par [n, 4] int32, contiguous")
        _lib.check(_lib.lib().mm_par_accum(_lib.ptr(done), _lib.ptr(reward), _lib.ptr(ep_stats), _lib.ptr(par),
                                           self.n, self.quota, _lib.ptr(self.counted), _lib.ptr(self.totals),
                                           _lib.stream_ptr()), "mm_par_accum")

    def words(self):
        """The 32 words as python ints (uint64).  Synchronises."""
        return [int(v) & (2**64 - 1) for v in self.totals.tolist()]

    def read(self):
        return result_from_par_words(self.words())


RECORD_DTYPE = np.dtype([("maze", "<i4"), ("episode", "<i4")] + [(name, "<i4") for name in _lib.ELOG_FIELDS])


class EpisodeLog:
    """One record per finished episode of ``venv`` (a VecMaze), the first ``quota`` episodes of every maze, written
    on the device (mm_elog_init / mm_elog_start / mm_elog_step, csrc/elog_kernels.hip): the maze, the outcome and
    par, when the key was found and by whom, when each agent learnt the exit, when the team became exit-ready, the
    cells each agent covered, its marks and stays (marlmaze.h: MM_ELOG_*).

    A finished maze's state is overwritten by its reset, so the log sits between the two.  Per env step::

        venv.step(actions, auto_reset=2, ...); log.step(actions, done, reward, ep_stats, par)
        venv.reset_done(...);                  log.start(select=done)

    and ``log.start()`` after the first ``venv.reset()``.  init(), start() and step() are stream-ordered launches (no
    allocation, no synchronisation); records() copies the log to the host.  ``log``: a caller-owned contiguous int32
    [n, quota, 16] tensor to write into (default: allocated here)."""

    def __init__(self, venv, quota=1, log=None):
        self.venv, self.n, self.quota = venv, int(venv.n), int(quota)
        if self.quota < 1:
            raise ValueError("EpisodeLog: quota >= 1")
        dev = venv.device
        self.state_words = int(_lib.lib().mm_elog_state_words(venv.stride))
        shape = (self.n, self.quota, _lib.ELOG_WORDS)
        if log is None:
            log = torch.empty(shape, dtype=torch.int32, device=dev)
        elif (log.dtype != torch.int32 or tuple(log.shape) != shape or not log.is_contiguous()
              or not log.is_cuda or log.data_ptr() % 16):
            raise ValueError(f"EpisodeLog: log must be a contiguous, 16-byte aligned int32 {list(shape)} tensor on {dev}")
        self.log = log
        self.counted = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.state = torch.empty(self.n * self.state_words, dtype=torch.int32, device=dev)  # the library's layout
        self.init()

    def init(self):
        _lib.check(_lib.lib().mm_elog_init(_lib.ptr(self.log), _lib.ptr(self.counted), _lib.ptr(self.state), self.n,
                                           self.quota, self.state_words, _lib.stream_ptr()), "mm_elog_init")

    def start(self, select=None):
        """After a reset: the mazes with select[m] != 0 ([n] uint8; None = all) begin a new episode."""
        if select is not None and (select.dtype != torch.uint8 or select.numel() != self.n
                                   or not select.is_contiguous() or not select.is_cuda):
            raise ValueError("EpisodeLog.start: select [n] uint8, contiguous, on the environment's device")
        _lib.check(_lib.lib().mm_elog_start(ctypes.byref(self.venv._desc), _lib.ptr(select), _lib.ptr(self.state),
                                            self.state_words, _lib.stream_ptr()), "mm_elog_start")

    def step(self, actions, done, reward, ep_stats, par=None):
        """After venv.step(actions, auto_reset=2, ...) and before venv.reset_done(): the step's actions [n, 2, 2]
        int8, done [n] u8, reward [n] f32 and ep_stats [n, 2] int32, and (optional) the par rows [n, 4] int32
        (VecMaze.par's) of the mazes that were stepped."""
        n = self.n
        if (actions.dtype != torch.int8 or done.dtype != torch.uint8 or reward.dtype != torch.float32
                or ep_stats.dtype != torch.int32 or actions.numel() != 4 * n or done.numel() != n
                or reward.numel() != n or ep_stats.numel() != 2 * n
                or not (actions.is_contiguous() and done.is_contiguous() and reward.is_contiguous()
                        and ep_stats.is_contiguous())
                or (par is not None and (par.dtype != torch.int32 or par.numel() != 4 * n
                                         or not par.is_contiguous()))):
            raise ValueError("EpisodeLog.step: actions [n, 2, 2] int8, done [n] uint8, reward [n] float32, ep_stats "
                             "[n, 2] int32, par [n, 4] int32 or None, contiguous")
        _lib.check(_lib.lib().mm_elog_step(ctypes.byref(self.venv._desc), _lib.ptr(actions), _lib.ptr(done),
                                           _lib.ptr(reward), _lib.ptr(ep_stats), _lib.ptr(par), self.quota,
                                           _lib.ptr(self.counted), _lib.ptr(self.state), self.state_words,
                                           _lib.ptr(self.log), _lib.stream_ptr()), "mm_elog_step")

    def maze_state(self):
        """The running state as an [n, state_words] view, row m = maze m's words (for tests; the words' meaning is
        the library's)."""
        return self.state.view(self.state_words, self.n).t()

    def records(self):
        """The written records as a numpy structured array (RECORD_DTYPE: maze, episode 0..quota-1 and the 16
        MM_ELOG_* words by name), in (maze, episode) order; rows never written (all -1) are dropped.  Synchronises."""
        log = self.log.cpu().numpy()
        maze, episode = np.nonzero((log != -1).any(-1))
        out = np.empty(len(maze), RECORD_DTYPE)
        out["maze"], out["episode"] = maze, episode
        for k, name in enumerate(_lib.ELOG_FIELDS):
            out[name] = log[maze, episode, k]
        return out


# the integer sums behind the behaviour statistics, in the order of the vector that DP ranks add up
BEHAVIOUR_SUMS = ("episodes", "key_found", "sum_t_key", "ready", "sum_t_ready", "solved_ready", "sum_t_exit",
                  "sum_covered", "sum_both", "sum_open", "fetched", "fetched_by_0", "sum_marks", "sum_stays")


def behaviour_sums(records):
    """Episode records (EpisodeLog.records()) -> the integer sums of BEHAVIOUR_SUMS, as a dict of python ints."""
    r = records
    i64 = lambda name: r[name].astype(np.int64)  # noqa: E731
    key, ready = r["T_KEY"] >= 0, r["T_READY"] >= 0
    out = ready & (r["SOLVED"] == 1)  # walked out after becoming exit-ready
    total = lambda v, sel=slice(None): int(v[sel].sum())  # noqa: E731
    return dict(
        episodes=len(r), key_found=int(key.sum()), sum_t_key=total(i64("T_KEY"), key), ready=int(ready.sum()),
        sum_t_ready=total(i64("T_READY"), ready), solved_ready=int(out.sum()),
        sum_t_exit=total(i64("LEN") - i64("T_READY"), out),
        sum_covered=total(i64("CELLS0") + i64("CELLS1") - i64("CELLS_BOTH")), sum_both=total(i64("CELLS_BOTH")),
        sum_open=total(i64("OPEN")), fetched=int((r["FETCHER"] >= 0).sum()), fetched_by_0=int((r["FETCHER"] == 0).sum()),
        sum_marks=total(i64("MARKS0") + i64("MARKS1")), sum_stays=total(i64("STAYS")))


def behaviour_from_sums(sums):
    """behaviour_sums' integers (a dict, or a sequence in BEHAVIOUR_SUMS order: one summed vector under DP) -> the
    behaviour statistics, every one a ratio of two of the sums.  Means over nothing are None.

    key_found_rate: episodes in which the key was picked up; mean_t_key: the step of the pickup, over those;
    mean_t_ready: the step at which both agents knew the exit and that the team has the key, over the episodes that
    got there; mean_t_exit: LEN - T_READY, the walk out, over the solved ones of those; coverage: cells stood on by
    either agent over the open cells; overlap: cells stood on by both over cells stood on by either; fetcher_share:
    agent 0's share of the pickups; marks_per_episode, stays_per_episode."""
    s = dict(sums) if isinstance(sums, dict) else dict(zip(BEHAVIOUR_SUMS, (int(v) for v in sums)))
    if sorted(s) != sorted(BEHAVIOUR_SUMS):
        raise ValueError(f"behaviour_from_sums: the {len(BEHAVIOUR_SUMS)} sums of BEHAVIOUR_SUMS expected")
    div = lambda a, b: (s[a] / s[b] if s[b] else None)  # noqa: E731
    return dict(
        key_found_rate=div("key_found", "episodes"), mean_t_key=div("sum_t_key", "key_found"),
        mean_t_ready=div("sum_t_ready", "ready"), mean_t_exit=div("sum_t_exit", "solved_ready"),
        coverage=div("sum_covered", "sum_open"), overlap=div("sum_both", "sum_covered"),
        fetcher_share=div("fetched_by_0", "fetched"), marks_per_episode=div("sum_marks", "episodes"),
        stays_per_episode=div("sum_stays", "episodes"))


def worst_records(records, k, by_par):
    """The k records with the largest LEN - PAR (by_par; an unrated maze's PAR <= 0 counts as 0) or the largest LEN,
    worst first, ties in (maze, episode) order."""
    key = records["LEN"].astype(np.int64) - (np.maximum(records["PAR"], 0) if by_par else 0)
    return records[np.argsort(-key, kind="stable")[:max(0, int(k))]]


def format_result(r):
    """One line for logs."""
    f = lambda v, p=2: "-" if v is None else f"{v:.{p}f}"  # noqa: E731
    line = (f"eval: {r['episodes']} episodes, {r['solved']} solved, {r['timeouts']} timed out "
            f"(success {f(r['success_rate'], 4)}); exit time {f(r['mean_len_solved'])} vs shortest path "
            f"{f(r['mean_shortest_solved'])} (ratio {f(r['mean_ratio'], 3)})")
    if "mean_par" in r and "mean_par_ratio" in r and "at_par" in r:
        line += f"; vs par {f(r['mean_par'])} (ratio {f(r['mean_par_ratio'], 3)}, {r['at_par']} at par)"
    if r.get("behaviour"):
        b = r["behaviour"]
        line += (f"; key found in {f(b['key_found_rate'], 4)} at t {f(b['mean_t_key'])}, exit-ready at t "
                 f"{f(b['mean_t_ready'])}, out in {f(b['mean_t_exit'])}, coverage {f(b['coverage'], 3)} "
                 f"(overlap {f(b['overlap'], 3)})")
    if "env_steps" in r and r.get("seconds"):
        line += f"; {r['env_steps']} env-steps in {r['seconds']:.2f} s = {r['env_steps'] / r['seconds']:.4g}/s"
    return line


def main(argv=None):
    """python -m marlmaze.evaluate: evaluate a checkpoint.  Returns the result dict (and prints it)."""
    ap = argparse.ArgumentParser(prog="python -m marlmaze.evaluate", description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="PPO.pth", help="checkpoint written by PPO.save_parameters (or the reference)")
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--size", type=int, default=10, help="maze side (default_size = (S, S))")
    ap.add_argument("--max-timestep", type=int, default=1200)
    ap.add_argument("--episodes", type=int, default=1, help="episodes per maze")
    ap.add_argument("--seed-base", type=int, default=0)
    ap.add_argument("--eval-seed", type=int, default=0)
    ap.add_argument("--sample", action="store_true", help="draw the actions (default: greedy)")
    ap.add_argument("--par", action="store_true", help="also rate the exit times against the mazes' par times")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line")
    ap.add_argument("--episode-log", metavar="PATH", help="log one record per episode on the device and save them "
                    "with numpy.savez (array `records`: seed, maze, episode and the MM_ELOG_* words)")
    ap.add_argument("--worst", type=int, default=0, metavar="K", help="print the K episodes with the largest len - par "
                    "(with --par; otherwise the largest len)")
    a = ap.parse_args(argv)
    from .PPO import PPO

    # (the agent only carries the networks and the env configuration: its training env is created on first use,
    # which never comes; evaluate() builds the mazes it steps)
    agent = PPO(2, n_envs=a.n_envs, model_path=a.model, load=False, verbose=False, save=False,
                env_config=dict(default_size=(a.size, a.size), max_timestep=a.max_timestep))
    if not agent.load_parameters():  # torch.load(weights_only=True)
        raise FileNotFoundError(a.model)
    res = agent.evaluate(episodes_per_env=a.episodes, greedy=not a.sample, seed_base=a.seed_base,
                         eval_seed=a.eval_seed, par=a.par, episode_log=bool(a.episode_log or a.worst > 0))
    res["mode"] = "sample" if a.sample else "greedy"
    records = res.pop("episode_log", None)  # an array: saved, not printed (`behaviour` stays in the result)
    if a.episode_log:
        np.savez(a.episode_log, records=records)
    print(json.dumps(res) if a.json else format_result(res), flush=True)
    for w in (worst_records(records, a.worst, a.par) if a.worst > 0 else ()):
        print(f"worst: seed {w['seed']} episode {w['episode']} len {w['LEN']} par {w['PAR']} t_key {w['T_KEY']} "
              f"t_ready {w['T_READY']}", flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
