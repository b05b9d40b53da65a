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

``PPO.evaluate`` drives both; ``python -m marlmaze.evaluate --model PPO.pth ...`` is the command line.
"""
import argparse
import json
import sys

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


def format_result(r):
    """One line for logs."""
    f = lambda v, p=2: "-" if v is None else f"{v:.{p}f}"  # noqa: E731
    line = (f"eval: {r['episodes']} episodes, {r['solved']} solved, {r['timeouts']} timed out "
            f"(success {f(r['success_rate'], 4)}); exit time {f(r['mean_len_solved'])} vs shortest path "
            f"{f(r['mean_shortest_solved'])} (ratio {f(r['mean_ratio'], 3)})")
    if "mean_par" in r and "mean_par_ratio" in r and "at_par" in r:
        line += f"; vs par {f(r['mean_par'])} (ratio {f(r['mean_par_ratio'], 3)}, {r['at_par']} at par)"
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
    a = ap.parse_args(argv)
    from .PPO import PPO

    # (the agent only carries the networks and the env configuration: its training env is created on first use,
    # which never comes; evaluate() builds the mazes it steps)
    agent = PPO(2, n_envs=a.n_envs, model_path=a.model, load=False, verbose=False, save=False,
                env_config=dict(default_size=(a.size, a.size), max_timestep=a.max_timestep))
    if not agent.load_parameters():  # torch.load(weights_only=True)
        raise FileNotFoundError(a.model)
    res = agent.evaluate(episodes_per_env=a.episodes, greedy=not a.sample, seed_base=a.seed_base,
                         eval_seed=a.eval_seed, par=a.par)
    res["mode"] = "sample" if a.sample else "greedy"
    print(json.dumps(res) if a.json else format_result(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
