"""The episode log (csrc/elog_kernels.hip, marlmaze.evaluate.EpisodeLog) and what stands on it.

Every value is an integer, so every comparison is exact.  The truth is a plain Python restatement of the sixteen
record words, kept here from VecMaze.agent_info(), maze_info(), layouts() and the action bytes after every step:
it does not go through the library.  No trained policy is needed: the actions are drawn by ops.act("sample") on zero
logits, uniform over the legal moves, a fair coin for the mark.

* the records and ``counted`` equal the host restatement on square, rectangular, mixed-size and largest mazes, with
  and without pre-generation, with and without a par buffer;
* the quota: rows past it stay -1, nothing is written behind the log;
* mm_elog_start's select leaves the other mazes' state bit for bit as it was;
* PPO.evaluate(episode_log=True) changes none of evaluate's keys and its records add up to them; the command line.
"""
import json

import numpy as np
import pytest
import torch

from marlmaze import _lib, ops
from marlmaze.evaluate import RECORD_DTYPE, EpisodeLog, behaviour_from_sums, behaviour_sums
from marlmaze.PPO import PPO
from marlmaze.vecmaze import VecMaze

pytestmark = pytest.mark.gpu

F = {name: k for k, name in enumerate(_lib.ELOG_FIELDS)}


# ---------------------------------------------------------------------------
# the host truth
# ---------------------------------------------------------------------------
class HostLog:
    """The sixteen words of marlmaze.h's MM_ELOG_* table, per maze, in plain Python."""

    def __init__(self, n, quota):
        self.n, self.quota = n, quota
        self.log = np.full((n, quota, _lib.ELOG_WORDS), -1, np.int32)
        self.counted = np.zeros(n, np.int32)
        self.cur = [None] * n

    def start(self, venv, select=None):
        agents, lays = venv.agent_info(), venv.layouts()
        for m in range(self.n):
            if select is not None and not select[m]:
                continue
            f = [int(agents[m, a]["flags"]) for a in (0, 1)]
            self.cur[m] = dict(
                seen=[{(int(agents[m, a]["x"]), int(agents[m, a]["y"]))} for a in (0, 1)], t_key=-1, fetcher=-1,
                t_know=[0 if f[a] & _lib.AF_KNOWS_END else -1 for a in (0, 1)], t_ready=-1,
                open=int((lays[m] != 1).sum()), marks=[0, 0], stays=0)

    def step(self, venv, actions, done, reward, stats, par):
        agents, mazes = venv.agent_info(), venv.maze_info()
        ready = _lib.AF_KNOWS_END | _lib.AF_TEAM_KEY
        for m in range(self.n):
            c, t = self.cur[m], int(mazes[m]["t"])
            f = [int(agents[m, a]["flags"]) for a in (0, 1)]
            for a in (0, 1):
                c["seen"][a].add((int(agents[m, a]["x"]), int(agents[m, a]["y"])))
                if c["t_know"][a] < 0 and f[a] & _lib.AF_KNOWS_END:
                    c["t_know"][a] = t
                c["marks"][a] += int(actions[m, a, 1] == 1)
                c["stays"] += int(actions[m, a, 0] == 4)
            if c["t_key"] < 0 and mazes[m]["kx"] < 0:
                c["t_key"] = t
                c["fetcher"] = 0 if f[0] & _lib.AF_HAS_KEY else 1 if f[1] & _lib.AF_HAS_KEY else -1
            if c["t_ready"] < 0 and f[0] & ready == ready and f[1] & ready == ready:
                c["t_ready"] = t
            if done[m] and self.counted[m] < self.quota:
                row = self.log[m, self.counted[m]]
                self.counted[m] += 1
                row[F["LEN"]], row[F["SHORTEST"]] = stats[m]
                row[F["SOLVED"]] = int(reward[m] == np.float32(1.0))
                row[F["PAR"]] = par[m, 0] if par is not None else -1
                row[F["T_KEY"]], row[F["FETCHER"]] = c["t_key"], c["fetcher"]
                row[F["T_KNOW0"]], row[F["T_KNOW1"]], row[F["T_READY"]] = c["t_know"][0], c["t_know"][1], c["t_ready"]
                row[F["CELLS0"]], row[F["CELLS1"]] = len(c["seen"][0]), len(c["seen"][1])
                row[F["CELLS_BOTH"]] = len(c["seen"][0] & c["seen"][1])
                row[F["OPEN"]] = c["open"]
                row[F["MARKS0"]], row[F["MARKS1"]], row[F["STAYS"]] = c["marks"][0], c["marks"][1], c["stays"]


def _drive(venv, elog, steps, key, host=None, with_par=False):
    """``steps`` env steps in evaluate's order around auto_reset=2, the host restatement (if any) alongside."""
    n = venv.n
    ml = torch.zeros((2 * n, 5), device="cuda")
    kl = torch.zeros(2 * n, device="cuda")
    stats = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    venv.reset()
    elog.start()
    par = venv.par() if with_par else None
    if host is not None:
        host.start(venv)
    for t in range(steps):
        act = ops.act(ml, kl, venv.masks.view(2 * n, 6), "sample", key, t)[0].view(n, 2, 2)
        _, _, rew, done = venv.step(act, auto_reset=2, ep_stats=stats)
        elog.step(act, done, rew, stats, par)
        if host is not None:
            dn = done.cpu().numpy()
            host.step(venv, act.cpu().numpy(), dn, rew.cpu().numpy(), stats.cpu().numpy(),
                      par.cpu().numpy() if with_par else None)
        venv.reset_done()
        elog.start(select=done)
        if with_par:
            venv.par(select=done, out=par)
        if host is not None and dn.any():
            host.start(venv, dn)
    assert (venv.status() & _lib.ST_BAD_MOVE == 0).all()  # (a small maze may have no cell for its key: MM_ST_GEN_FAIL)


# Configuration 0's seeds and max_timestep: the CPU oracle (oracle/env.py, OracleEnv(48, default_size=(4, 4),
# max_timestep=40, seeds=range(48)), legal moves drawn uniformly, marks by a fair coin, 85 steps, five generator seeds)
# gave 8 to 13 solved and 83 to 88 timed-out episodes among each maze's first two, the key found in 29 to 36 of
# them; seeds 100.. and 1000.. gave 4 to 9 solved.  So seeds 0..47 at 40 steps hold all three kinds.
CONFIGS = [
    dict(n=48, quota=2, steps=85, with_par=True, env=dict(default_size=(4, 4), max_timestep=40)),  # 48: tail lanes
    dict(n=33, quota=1, steps=45, env=dict(default_size=(3, 5), max_timestep=40)),  # w != h
    dict(n=40, quota=2, steps=65, env=dict(rand_sizes=True, rand_range=(3, 6), max_timestep=30)),  # a width per maze
    dict(n=3, quota=1, steps=14, env=dict(default_size=(21, 21), max_timestep=12)),  # stride 1681: 53-word bitmaps
    dict(n=48, quota=2, steps=50, env=dict(default_size=(4, 4), max_timestep=20, pregen=False)),
]
IDS = ["4x4-par", "3x5", "rand-3..6", "21x21", "no-pregen"]


@pytest.mark.parametrize("k", range(len(CONFIGS)), ids=IDS)
def test_records_equal_host_restatement(k):
    cfg = CONFIGS[k]
    n, quota = cfg["n"], cfg["quota"]
    venv = VecMaze(n, seeds=np.arange(n, dtype=np.uint64), **cfg["env"])
    elog, host = EpisodeLog(venv, quota), HostLog(n, quota)
    if k == 3:  # the last bitmap word is partial
        assert venv.stride == 1681 and elog.state_words - _lib.lib().mm_elog_state_words(1) == 2 * (53 - 1)
    _drive(venv, elog, cfg["steps"], 11 + k, host, cfg.get("with_par", False))
    got, counted = elog.log.cpu().numpy(), elog.counted.cpu().numpy()
    rec = elog.records()
    print(f"{IDS[k]}: {len(rec)} records, solved {int(rec['SOLVED'].sum())}, key found {int((rec['T_KEY'] >= 0).sum())}, "
          f"exit-ready {int((rec['T_READY'] >= 0).sum())}, rows differing {int((got != host.log).any(-1).sum())}")
    assert np.array_equal(counted, host.counted)
    assert np.array_equal(got, host.log)
    assert (counted == quota).all()  # the run was long enough for every maze
    # records(): the written rows, named, in (maze, episode) order
    assert rec.dtype == RECORD_DTYPE and len(rec) == n * quota
    assert np.array_equal(rec["maze"], np.repeat(np.arange(n), quota))
    assert np.array_equal(rec["episode"], np.tile(np.arange(quota), n))
    for name, w in F.items():
        assert np.array_equal(rec[name], host.log[:, :, w].reshape(-1)), name
    if k == 0:  # the parity above is not one over an empty set
        assert (rec["SOLVED"] == 1).any() and (rec["SOLVED"] == 0).any() and (rec["T_KEY"] >= 0).any()
        assert (rec["T_READY"] >= 0).any() and (rec["PAR"] > 0).any()
    else:
        assert (rec["PAR"] == -1).all()
    if k == 2:
        assert len(set(rec["OPEN"].tolist())) > 1  # mazes of several sizes
    # what every record obeys
    assert (rec["CELLS_BOTH"] <= np.minimum(rec["CELLS0"], rec["CELLS1"])).all()
    assert (rec["CELLS0"] + rec["CELLS1"] - rec["CELLS_BOTH"] <= rec["OPEN"]).all()
    # (a maze generated without a key reports it gone at t = 1 with no fetcher)
    assert (rec["T_KEY"][rec["FETCHER"] >= 0] >= 1).all() and (rec["T_READY"] <= rec["LEN"]).all()
    b = behaviour_from_sums(behaviour_sums(rec))
    assert 0 < b["coverage"] <= 1 and 0 <= b["overlap"] <= 1


def test_quota_and_guard():
    n, quota, guard = 70, 2, 4096
    venv = VecMaze(n, seeds=np.arange(n, dtype=np.uint64) + np.uint64(500), default_size=(3, 3), max_timestep=6)
    words = n * quota * _lib.ELOG_WORDS
    buf = torch.full((words + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    elog = EpisodeLog(venv, quota, log=buf[:words].view(n, quota, _lib.ELOG_WORDS))
    assert (buf[:words] == -1).all() and (buf[words:] == 0x5A5A5A5A).all()
    _drive(venv, elog, 6, 3)  # max_timestep steps: every maze has finished an episode, few of them two
    counted = elog.counted.cpu().numpy()
    first = elog.log.cpu().numpy()
    assert (counted >= 1).all() and (counted < quota).any()
    written = counted[:, None] > np.arange(quota)[None, :]  # rows up to counted hold a record, the others -1
    assert (first[written][:, F["LEN"]] > 0).all() and (first[~written] == -1).all()
    _drive_on(venv, elog, 40, 3)  # at least six more episodes per maze: far past the quota
    assert (venv.maze_info()["episodes"] >= 7).all()
    log = elog.log.cpu().numpy()
    assert (elog.counted.cpu().numpy() == quota).all()
    assert np.array_equal(log[written], first[written]) and (log[:, :, F["LEN"]] > 0).all()
    assert len(elog.records()) == n * quota
    assert (buf[words:] == 0x5A5A5A5A).all()
    with pytest.raises(ValueError):
        EpisodeLog(venv, 0)


def _drive_on(venv, elog, steps, key):
    """More steps of a running environment (no reset before)."""
    n = venv.n
    ml, kl = torch.zeros((2 * n, 5), device="cuda"), torch.zeros(2 * n, device="cuda")
    stats = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    for t in range(steps):
        act = ops.act(ml, kl, venv.masks.view(2 * n, 6), "sample", key, 1000 + t)[0].view(n, 2, 2)
        _, _, rew, done = venv.step(act, auto_reset=2, ep_stats=stats)
        elog.step(act, done, rew, stats)
        venv.reset_done()
        elog.start(select=done)


def test_start_select_leaves_other_mazes_untouched():
    n = 130
    venv = VecMaze(n, seeds=np.arange(n, dtype=np.uint64) + np.uint64(900), default_size=(4, 4), max_timestep=200)
    elog = EpisodeLog(venv, 1)
    _drive(venv, elog, 12, 9)  # twelve steps into the first episodes: visited cells, marks, milestones
    before = elog.maze_state().clone()
    fresh = EpisodeLog(venv, 1)
    fresh.start()  # what a start makes of every maze as it stands
    want = fresh.maze_state().clone()
    assert before.shape == (n, elog.state_words) and (before != want).any(1).sum() > n // 2
    rng = np.random.default_rng(4)
    sel = rng.integers(0, 3, n).astype(np.uint8)  # 0 = leave; 1 and 2 = start
    sel[[0, 63, 64, 129]] = [1, 0, 2, 0]
    select = torch.as_tensor(sel).cuda()
    elog.start(select=select)
    after = elog.maze_state()
    chosen = torch.as_tensor(sel != 0).cuda()
    assert torch.equal(after[~chosen], before[~chosen])
    assert torch.equal(after[chosen], want[chosen])
    assert 20 < int(chosen.sum()) < n - 20


def test_arguments_are_validated():
    n = 8
    venv = VecMaze(n, default_size=(3, 3), max_timestep=10)
    venv.reset()
    elog = EpisodeLog(venv, 1)
    act = torch.zeros((n, 2, 2), dtype=torch.int8, device="cuda")
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rew = torch.zeros(n, dtype=torch.float32, device="cuda")
    stats = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    par = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    elog.step(act, done, rew, stats, par)
    for bad in ((act.int(), done, rew, stats, par), (act, done.bool(), rew, stats, par), (act, done, rew.double(), stats, par),
                (act, done, rew, stats.long(), par), (act, done, rew, stats, par.long()), (act[:4], done, rew, stats, par),
                (act, done, rew, stats.t(), par), (act, done, rew, stats, par[:, :2]),
                (act, done[:4], rew, stats, None)):
        with pytest.raises(ValueError):
            elog.step(*bad)
    for bad in (done.bool(), done[:4], torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError):
            elog.start(select=bad)
    with pytest.raises(ValueError):
        EpisodeLog(venv, 1, log=torch.zeros((n, 2, 16), dtype=torch.int32, device="cuda"))
    L = _lib.lib()  # the C ABI refuses a state of the wrong size
    import ctypes
    assert L.mm_elog_start(ctypes.byref(venv._desc), None, _lib.ptr(elog.state), elog.state_words + 1,
                           _lib.stream_ptr()) == -1


# ---------------------------------------------------------------------------
# PPO.evaluate(episode_log=True) and the command line
# ---------------------------------------------------------------------------
def _agent(**kw):
    kw.setdefault("load", False)
    kw.setdefault("verbose", False)
    kw.setdefault("save", False)
    return PPO(2, **kw)


def test_evaluate_with_the_log_equals_evaluate_without():
    n, E = 32, 2
    cfg = dict(default_size=(4, 4), max_timestep=40)
    ag = _agent(n_envs=n)
    kw = dict(episodes_per_env=E, greedy=True, n_envs=n, env_config=cfg, seed_base=0)
    plain = ag.evaluate(par=True, **kw)
    res = ag.evaluate(par=True, episode_log=True, **kw)
    for key in plain:  # the auto_reset=2 path changes nothing
        if key != "seconds":
            assert res[key] == plain[key], key
    assert set(res) - set(plain) == {"episode_log", "behaviour"}
    rec = res["episode_log"]
    print(f"{len(rec)} records, solved {int(rec['SOLVED'].sum())}, behaviour {res['behaviour']}")
    assert len(rec) == res["episodes"] == n * E
    assert int(rec["LEN"].sum()) == round(res["mean_len"] * res["episodes"])
    assert int(rec["SOLVED"].sum()) == res["solved"]
    assert np.array_equal(rec["seed"], rec["maze"].astype(np.uint64)) and set(rec.dtype.names) == set(
        RECORD_DTYPE.names) | {"seed"}
    v = VecMaze(n, seeds=np.arange(n, dtype=np.uint64), **cfg)
    v.reset()
    first = rec[rec["episode"] == 0]
    assert np.array_equal(first["maze"], np.arange(n))
    assert np.array_equal(first["PAR"], v.par().cpu().numpy()[:, 0])
    assert res["behaviour"] == behaviour_from_sums(behaviour_sums(rec))
    # rated episodes: the records' excess over par is the totals'
    rated = rec[(rec["SOLVED"] == 1) & (rec["PAR"] > 0)]
    assert len(rated) == res["par_episodes"]
    assert res["max_excess"] == (int((rated["LEN"] - rated["PAR"]).max()) if len(rated) else 0)
    # without par: the same records with PAR = -1; without the flag: neither key
    nopar = ag.evaluate(episode_log=True, **kw)["episode_log"]
    assert (nopar["PAR"] == -1).all()
    for name in rec.dtype.names:
        if name != "PAR":
            assert np.array_equal(nopar[name], rec[name]), name
    off = ag.evaluate(**kw)
    assert "episode_log" not in off and "behaviour" not in off


def test_cli_episode_log_and_worst(tmp_path, capsys):
    from marlmaze import evaluate

    path, out = str(tmp_path / "PPO.pth"), str(tmp_path / "episodes.npz")
    _agent(n_envs=32, model_path=path).save_parameters()
    ret = evaluate.main(["--model", path, "--n-envs", "32", "--size", "4", "--max-timestep", "40", "--par",
                         "--episode-log", out, "--worst", "3", "--json"])
    lines = capsys.readouterr().out.splitlines()
    res = json.loads([ln for ln in lines if ln.startswith("{")][-1])  # valid JSON: the records are not in it
    assert "episode_log" not in res and "episode_log" not in ret and res["episodes"] == 32
    assert set(res["behaviour"]) == set(behaviour_from_sums([0] * 14))
    with np.load(out) as z:
        rec = z["records"]
    assert len(rec) == 32 and set(RECORD_DTYPE.names) | {"seed"} == set(rec.dtype.names)
    assert int(rec["SOLVED"].sum()) == res["solved"] and res["behaviour"] == behaviour_from_sums(behaviour_sums(rec))
    worst = [ln for ln in lines if ln.startswith("worst: ")]
    key = rec["LEN"].astype(np.int64) - np.maximum(rec["PAR"], 0)
    top = rec[np.argsort(-key, kind="stable")[:3]]
    assert worst == [f"worst: seed {w['seed']} episode {w['episode']} len {w['LEN']} par {w['PAR']} t_key {w['T_KEY']} "
                     f"t_ready {w['T_READY']}" for w in top]
    evaluate.main(["--model", path, "--n-envs", "32", "--size", "4", "--max-timestep", "40", "--worst", "2"])
    text = capsys.readouterr().out
    assert "; key found in " in text and text.count("worst: ") == 2 and " par -1 " in text
