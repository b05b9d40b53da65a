"""Policy evaluation: whole episodes on many mazes at once, counted on the device.

``EvalTotals`` wraps the device buffers of mm_eval_init / mm_eval_accum (csrc/eval_kernels.hip): after every
env step, every maze that finished an episode -- and has not yet contributed its quota of episodes -- adds it
to 32 integer words (episodes, solved, timeouts, sums of lengths and shortest paths, min / max, a histogram of
exit time over shortest path).  Every maze contributes its FIRST ``quota`` episodes and nothing else, so the
result is a per-maze average: without the quota, mazes with short episodes would finish more of them inside
any fixed number of steps and bias the success rate upwards.

``ParTotals`` is its counterpart against par (mm_par_init / mm_par_accum, the same file and the same 32-word
shape): the exit time of every counted solved episode over the par time of its maze, the length of the shortest
possible solving episode (VecMaze.par).  The floor of that ratio is 1.0, which the ratio over the shortest
start -> end path cannot reach: the key never lies on that path.

``EpisodeLog`` keeps what the totals cannot say: one record per counted episode (mm_elog_init / mm_elog_start /
mm_elog_step, csrc/elog_kernels.hip) -- which maze, its outcome and par, when the key was found and by whom, when
each agent learnt the exit, when the team became exit-ready, the cells each agent covered, its marks and stays.
``behaviour_sums`` / ``behaviour_from_sums`` reduce the records to statistics, each a ratio of two integer sums.

``evaluate_policy`` drives all three (``PPO.evaluate`` is a call of it): the look at the GEMMs' range flag and
the repeat at x3, the stepping loop (``_run``, one step sequence with or without par and the log), the reduction
of the words over DP ranks (``reduce_words``, from the tables EVAL_EXTREMES / PAR_EXTREMES) and the result dict.
``python -m marlmaze.evaluate --model PPO.pth ...`` is the command line.
"""
import argparse
import collections
import ctypes
import json
import sys
import time
import warnings

import numpy as np
import torch
from numpy.lib import recfunctions

from . import _lib, x3
from .vecmaze import VecMaze

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


def _check_step_args(who, n, done, reward, ep_stats, par=None, actions=None):
    """ValueError unless one env step's tensors are what the accumulate kernels read for ``n`` mazes: done [n]
    uint8, reward [n] float32, ep_stats [n, 2] int32 and, where given, par [n, 4] int32 and actions [n, 2, 2] int8,
    each contiguous.  Called before anything is launched (and once per step: one flat condition)."""
    if (done.dtype != torch.uint8 or reward.dtype != torch.float32 or ep_stats.dtype != torch.int32
            or done.numel() != n or reward.numel() != n or ep_stats.numel() != 2 * n
            or not (done.is_contiguous() and reward.is_contiguous() and ep_stats.is_contiguous())
            or (par is not None and (par.dtype != torch.int32 or par.numel() != 4 * n or not par.is_contiguous()))
            or (actions is not None and (actions.dtype != torch.int8 or actions.numel() != 4 * n
                                         or not actions.is_contiguous()))):
        raise ValueError(f"{who}: done [n] uint8, reward [n] float32, ep_stats [n, 2] int32 and, where taken, par "
                         "[n, 4] int32 and actions [n, 2, 2] int8, contiguous")


class _Totals:
    """32 uint64 words of totals on the device over ``n`` mazes, ``quota`` episodes per maze, with the ``counted``
    array of the quota rule.  A subclass names its mm_*_init entry point, gives the result function of its words
    and adds accum().

    init() and accum() are stream-ordered launches (no allocation, no synchronisation); words() and read()
    copy the 32 words to the host."""

    _init = _result = None

    def __init__(self, n, quota=1, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.quota = int(n), int(quota)
        self.totals = torch.empty(_lib.EVAL_WORDS, dtype=torch.int64, device=device)  # uint64 words
        self.counted = torch.empty(self.n, dtype=torch.int32, device=device)
        self.init()

    def init(self):
        _lib.check(getattr(_lib.lib(), self._init)(_lib.ptr(self.totals), _lib.ptr(self.counted), self.n,
                                                   _lib.stream_ptr()), self._init)

    def words(self):
        """The 32 words as python ints (uint64).  Synchronises."""
        return [int(v) & (2**64 - 1) for v in self.totals.tolist()]

    def read(self):
        return self._result(self.words())


class EvalTotals(_Totals):
    """Device totals of an evaluation over ``n`` mazes, ``quota`` episodes per maze."""

    _init, _result = "mm_eval_init", staticmethod(result_from_words)

    def accum(self, done, reward, ep_stats):
        """One env step's done [n] u8, reward [n] f32 and ep_stats [n, 2] int32 (VecMaze.step's)."""
        _check_step_args("EvalTotals.accum", self.n, done, reward, ep_stats)
        _lib.check(_lib.lib().mm_eval_accum(_lib.ptr(done), _lib.ptr(reward), _lib.ptr(ep_stats), self.n, self.quota,
                                            _lib.ptr(self.counted), _lib.ptr(self.totals), _lib.stream_ptr()),
                   "mm_eval_accum")


class ParTotals(_Totals):
    """Device totals of exit time against par over ``n`` mazes, ``quota`` episodes per maze (EvalTotals' shape,
    with a ``counted`` array of its own)."""

    _init, _result = "mm_par_init", staticmethod(result_from_par_words)

    def accum(self, done, reward, ep_stats, par):
        """One env step's done [n] u8, reward [n] f32 and ep_stats [n, 2] int32 (VecMaze.step's), and the par
        rows [n, 4] int32 (VecMaze.par's) of the mazes that were stepped."""
        _check_step_args("ParTotals.accum", self.n, done, reward, ep_stats, par)
        _lib.check(_lib.lib().mm_par_accum(_lib.ptr(done), _lib.ptr(reward), _lib.ptr(ep_stats), _lib.ptr(par),
                                           self.n, self.quota, _lib.ptr(self.counted), _lib.ptr(self.totals),
                                           _lib.stream_ptr()), "mm_par_accum")


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
        _check_step_args("EpisodeLog.step", self.n, done, reward, ep_stats, par, actions)
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


# The words that are not sums, by kind; every other word of the 32 is a sum.  Nothing else says which is which
# on the host: reduce_words reads these two tables
EVAL_EXTREMES = {_lib.EV_MIN_LEN_SOLVED: "min", _lib.EV_MAX_LEN_SOLVED: "max"}
PAR_EXTREMES = {_lib.PAR_MAX_EXCESS: "max"}


def _reduce(words, extremes, dp, device):
    """One set of 32 words over all ranks, in two collectives: a SUM of the sums and a MAX of the extremes, a
    minimum travelling as the maximum of its complement (0 from a rank whose min word is still NONE_MIN)."""
    sums = torch.tensor([0 if k in extremes else v for k, v in enumerate(words)], dtype=torch.int64, device=device)
    ext = torch.tensor([words[k] if kind == "max" else (2**62 - words[k] if words[k] != NONE_MIN else 0)
                        for k, kind in extremes.items()], dtype=torch.int64, device=device)
    out = dp.allreduce_sum(sums).tolist()
    for (k, kind), v in zip(extremes.items(), dp.allreduce_max(ext).tolist()):
        out[k] = v if kind == "max" else (2**62 - v if v > 0 else NONE_MIN)
    return out


def reduce_words(words, pwords, dp, device):
    """This rank's 32 words and its 32 words against par (or None, on every rank alike) -> those of all ranks'
    mazes.  Every rank issues the same collectives in the same order: two for the totals, then two for par if
    there is par.  Under DP.single() the input is returned as it is."""
    if not dp.active:
        return words, pwords
    return (_reduce(words, EVAL_EXTREMES, dp, device),
            None if pwords is None else _reduce(pwords, PAR_EXTREMES, dp, device))


# one evaluation run on this rank: the steps taken, its 32 words, its 32 words against par or None, the recorded
# steps or None, the stepping loop's start time, and its episode records or None
EvalRun = collections.namedtuple("EvalRun", "steps words pwords record t0 records")


def _run(agent, n, E, seeds, kw, mode, key, poll, record, par, episode_log):
    """One evaluation at the actor's current GEMM precision on a fresh VecMaze -> EvalRun.  The side-stream maze
    pre-generation is queued once per poll window, as the rollout queues it once per horizon
    (VecMaze.defer_pregen)."""
    dev, dp = agent.device, agent.dp
    venv = VecMaze(n, seeds=seeds, device=dev, **kw)
    max_steps = E * venv.max_timestep  # k_step ends an episode at t >= max_timestep
    obs = torch.empty((n, 2, 65), dtype=torch.float32, device=dev)
    masks = torch.empty((n, 2, 6), dtype=torch.uint8, device=dev)
    act = torch.empty((n, 2, 2), dtype=torch.int8, device=dev)
    rowlp = torch.empty(2 * n, dtype=torch.float32, device=dev)
    rew = torch.empty(n, dtype=torch.float32, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    stats = torch.empty((n, 2), dtype=torch.int32, device=dev)
    tot = EvalTotals(n, E, device=dev)
    head_w, head_b = agent.actor.heads()
    rec = dict(actions=[], done=[], reward=[]) if record else None
    venv.reset(obs=obs, masks=masks)
    partot = parbuf = None
    if par:  # every maze's par time, refreshed below whenever a maze is replaced by its next one
        partot = ParTotals(n, E, device=dev)
        parbuf = venv.par()
    elog = None
    if episode_log:  # the first episodes' spawn cells and open cells
        elog = EpisodeLog(venv, E)
        elog.start()
    torch.cuda.synchronize(dev)  # the caller's `seconds` is the stepping loop's: the mazes exist
    t0, t = time.perf_counter(), 0
    venv.defer_pregen = True
    try:
        with x3.cached_packs():  # the weights are fixed: packed once
            while True:
                agent.actor.act(obs.view(2 * n, 65), head_w, head_b, masks.view(2 * n, 6), mode, key, t,
                                actions=act.view(2 * n, 2), logp=rowlp)
                # with the log, the finished mazes are only queued (auto_reset=2) and reset below, after the log
                # has seen their last state; without it the step resets them itself, in the same launch
                venv.step(act, auto_reset=2 if elog else True, obs=obs, masks=masks, reward=rew, done=done,
                          ep_stats=stats)
                tot.accum(done, rew, stats)
                if par:  # against the par of the maze that just finished
                    partot.accum(done, rew, stats, parbuf)
                if elog:
                    elog.step(act, done, rew, stats, parbuf)
                    venv.reset_done(obs=obs, masks=masks)
                    elog.start(select=done)
                if par:  # the par of the maze that the reset installed
                    venv.par(select=done, out=parbuf)
                t += 1
                if rec is not None:
                    rec["actions"].append(act.clone())
                    rec["done"].append(done.clone())
                    rec["reward"].append(rew.clone())
                if t % poll and t < max_steps:
                    continue
                venv.defer_pregen = False  # the window's finished mazes get their next mazes generated
                venv.flush_pregen()
                venv.defer_pregen = True
                words = tot.words()  # the host synchronisation
                count = torch.tensor([words[_lib.EV_EPISODES]], dtype=torch.int64, device=dev)
                if int(dp.allreduce_sum(count)) == n * E * dp.world:  # every rank stops at the same step
                    break
                if t >= max_steps:
                    raise RuntimeError(f"evaluate: {int(count)} of {n * E * dp.world} episodes after {t} "
                                       f"steps (max_timestep {venv.max_timestep})")
    finally:
        venv.defer_pregen = False
        venv.flush_pregen()
        venv._quiesce_pregen()  # the side stream's generation ends before the buffers go
    if rec is not None:
        rec = {k: torch.stack(v) for k, v in rec.items()}
    erec = None
    if elog:
        erec = elog.records()
        erec = recfunctions.append_fields(erec, "seed", seeds[erec["maze"]], usemask=False)
    return EvalRun(t, words, partot.words() if par else None, rec, t0, erec)


@torch.no_grad()
def evaluate_policy(agent, episodes_per_env=1, greedy=True, n_envs=None, env_config=None, seed_base=0, eval_seed=0,
                    poll=16, record=False, par=False, episode_log=False):
    """How good is the policy of ``agent`` (a PPO; ``PPO.evaluate`` is this function): ``episodes_per_env`` whole
    episodes on each of ``n_envs`` fresh mazes (seeds ``seed_base + rank n + i``; configuration ``env_config``,
    else the agent's), every agent taking its most likely action (``greedy``) or drawing one (Philox key
    ``eval_seed``, counter = the step).  Per step: front-end, trunk, mm_head_act, the env step with auto-reset,
    mm_eval_accum; the totals are read every ``poll`` steps and the run ends when every maze has contributed its
    episodes (each maze its first ``episodes_per_env``) -- at the latest after ``episodes_per_env * max_timestep``
    steps, where an episode is cut off.  Under DP the totals are those of all ranks' mazes (reduce_words).

    ``par``: also rate every counted solved episode against the par time of its maze, the length of the
    shortest possible solving episode (VecMaze.par; mm_par_accum after mm_eval_accum, then mm_env_par for the
    mazes that finished and hold their next maze); the result gains result_from_par_words' keys.  Off (the
    default), nothing is launched and nothing is added.

    ``episode_log``: also write one record per counted episode on the device (EpisodeLog: which maze, the outcome
    and par, when the key was found and by whom, when each agent learnt the exit, when the team became exit-ready,
    the cells covered, marks and stays).  The finished mazes' state is gone once they are reset, so the step
    becomes: the env step with its finished mazes only queued (auto_reset=2), mm_eval_accum, mm_par_accum,
    mm_elog_step, the queued resets, mm_elog_start and mm_env_par for the mazes that finished -- the same mazes,
    actions and totals as without it.  The result gains ``episode_log``, this rank's records as a numpy structured
    array (EpisodeLog.records() plus ``seed``, the maze's seed; PAR is -1 without ``par``), and ``behaviour``,
    behaviour_from_sums' statistics over all ranks' records.  Off (the default), the step is the one above,
    nothing is launched and nothing is added.

    Returns result_from_words' dict plus ``env_steps`` and ``seconds``; with ``record`` also a dict of the
    per-step ``actions`` [T, n, 2, 2], ``done`` [T, n] and ``reward`` [T, n] of this rank (for small n).
    Training does not notice the call: it uses an environment and buffers of its own and leaves the rollout's
    environment, buffers, sampler offset, the range-guard state and every random generator as they are."""
    n, E = int(n_envs if n_envs is not None else agent.n_envs), int(episodes_per_env)
    if n < 1 or E < 1:
        raise ValueError("evaluate needs n_envs >= 1 and episodes_per_env >= 1")
    kw = dict(env_config) if env_config is not None else agent._env_kwargs()
    kw.pop("seed_base", None)
    dev, dp, actor = agent.device, agent.dp, agent.actor
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(int(seed_base) + dp.rank * n)
    args = (agent, n, E, seeds, kw, "greedy" if greedy else "sample", int(eval_seed) + 7919 * dp.rank,
            max(1, int(poll)), bool(record), bool(par), bool(episode_log))

    # The fp16-plane GEMMs (x2, f16) raise the library's range flag, which belongs to the rollout and the
    # update (PPO._range_guarded).  It is only looked at here, never cleared while it carries their state: raised
    # already -> this run uses x3 (which leaves it alone); raised BY this run -> back to clear, its state
    # before, and the run is repeated at x3, as the update does.  Under DP both decisions are taken from the
    # MAX over ranks (DP.raised_on_any_rank, the update's rule): every rank runs at the same precision and issues
    # the same collectives
    guarded = agent.flat is not None and actor.gemm_prec != "x3"
    prec = actor.gemm_prec
    try:
        if guarded and dp.raised_on_any_rank(x3.range_flag(clear=False))[0]:
            actor.gemm_prec = "x3"
            guarded = False
        run = _run(*args)
        if guarded:
            mine = x3.range_flag(clear=False)
            if dp.raised_on_any_rank(mine)[0]:
                if int(mine):  # raised by this run (it was clear before): clear again
                    x3.range_flag(clear=True)
                warnings.warn(f"marlmaze: a {prec} GEMM operand of the evaluation reached |x| >= 2^15 (fp16 "
                              "planes): the evaluation is repeated at x3")
                actor.gemm_prec = "x3"
                run = _run(*args)
        seconds = time.perf_counter() - run.t0
    finally:
        actor.gemm_prec = prec
    words, pwords = reduce_words(run.words, run.pwords, dp, dev)
    res = result_from_words(words)
    if pwords is not None:
        res.update(result_from_par_words(pwords))
    if run.records is not None:  # this rank's records; the statistics from one summed vector of all ranks' integers
        sums = behaviour_sums(run.records)
        if dp.active:
            sums = dp.allreduce_sum(torch.tensor([sums[k] for k in BEHAVIOUR_SUMS], dtype=torch.int64,
                                                 device=dev)).tolist()
        res["episode_log"] = run.records
        res["behaviour"] = behaviour_from_sums(sums)
    res["env_steps"] = n * run.steps * dp.world
    res["seconds"] = seconds
    return (res, run.record) if record else res


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
