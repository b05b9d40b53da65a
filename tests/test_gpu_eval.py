"""Policy evaluation on the GPU: the greedy / sampling action kernels (mm_head_act, mm_act), the episode totals
(mm_eval_init, mm_eval_accum) and PPO.evaluate on top of them.

* the greedy head is torch.argmax / (logit > 0) on mm_heads_fwd's logits, exactly;
* the sampler, in its plain and its mode form, gives the recorded outputs of tests/golden/sampler_pinned.npz, bit
  for bit;
* the totals equal a plain numpy loop, word for word;
* PPO.evaluate's recorded actions, replayed on the C oracle, give the same episodes and totals;
* training does not notice an evaluation; greedy evaluation is reproducible; DP sums; the command line.
"""
import hashlib
import json
import os
import random
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from marlmaze import _lib, ops
from marlmaze.evaluate import EvalTotals
from marlmaze.PPO import PPO
from oracle.env import OracleEnv

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 1e-6  # tests/test_gpu_rl.py::test_sampler_logp_and_legality's bar
SHAPES = [(M, K) for M in (1, 2, 31, 33, 4097) for K in (8, 264)]
DIGEST_ONLY = {(4097, 264)}  # sampler_pinned.npz holds this shape's arrays as SHA-256 digests (size)


def _agent(**kw):
    kw.setdefault("load", False)
    kw.setdefault("verbose", False)
    kw.setdefault("save", False)
    return PPO(2, **kw)


def _load(agent, fx, prefix_a="actor/", prefix_c="critic/"):  # tests/test_gpu_ppo.py::_load
    agent.actor.load_state_dict({k[len(prefix_a):]: torch.as_tensor(fx[k]) for k in fx.files if k.startswith(prefix_a)})
    agent.critic.load_state_dict({k[len(prefix_c):]: torch.as_tensor(fx[k]) for k in fx.files
                                  if k.startswith(prefix_c)})


# ---------------------------------------------------------------------------
# 1, 2: the action kernels
# ---------------------------------------------------------------------------
def _head_inputs(M, K):
    """h, W, b, masks with: head rows 1 and 3 identical with equal (high) biases -> exact ties that often win;
    a zero mark bias and an all-zero h row -> a mark logit of exactly 0; rows with one legal move, with the mark
    disallowed, with no legal move."""
    rng = np.random.default_rng(1000 * M + K)
    h = rng.normal(0, 1, (M, K)).astype(np.float32)
    w = (rng.normal(0, 1, (6, K)) * 2 / np.sqrt(K)).astype(np.float32)
    b = np.clip(rng.normal(0, 1, 6), -2, 2).astype(np.float32)
    w[3] = w[1]
    b[1] = b[3] = 3.0
    b[5] = 0.0
    mk = rng.random((M, 6)) < 0.75
    h[0] = 0.0  # row 0: logits = biases: the tie (1, 3) is the maximum, the mark logit is exactly 0
    mk[0] = True
    if M > 1:
        mk[1] = [False, False, True, False, False, True]  # one legal move
    if M > 2:
        mk[2, 5] = False  # mark disallowed
        mk[3, :5] = False  # no legal move
        mk[4] = [True, False, False, True, True, True]  # the tie's lower index illegal
    return h, w, b, mk


def _heads_fwd(h, w, b):
    M, K = h.shape
    out = torch.empty((M, 6), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().mm_heads_fwd(_lib.ptr(h), K, K, _lib.ptr(w), _lib.ptr(b), M, _lib.ptr(out),
                                       _lib.stream_ptr()), "mm_heads_fwd")
    return out


@pytest.mark.parametrize("M,K", SHAPES)
def test_greedy_head_is_argmax(M, K):
    h, w, b, mk = _head_inputs(M, K)
    dh, dw, db = (torch.as_tensor(x).cuda() for x in (h, w, b))
    dmk = torch.as_tensor(mk.astype(np.uint8)).cuda()
    ref_logits = _heads_fwd(dh, dw, db)
    logits = torch.full((M, 6), float("nan"), device="cuda")
    a, lp, jl = ops.head_act(dh, dw, db, dmk, mode="greedy", logits=logits)
    assert torch.equal(logits, ref_logits)  # bitwise: the same per-lane arithmetic
    z = ref_logits.cpu().numpy()
    a, lp, jl = a.cpu().numpy().astype(np.int64), lp.cpu().numpy(), jl.cpu().numpy()
    legal = mk[:, :5].any(1)
    masked = np.where(mk[:, :5], z[:, :5], -np.inf)
    want_move = np.where(legal, np.argmax(masked, 1), 4)  # first occurrence of the maximum
    want_mark = mk[:, 5] & (z[:, 5] > 0)
    print(f"M={M} K={K}: moves differing {int((a[:, 0] != want_move).sum())}, marks differing "
          f"{int((a[:, 1] != want_mark).sum())}")
    assert np.array_equal(a[:, 0], want_move)
    assert np.array_equal(a[:, 1], want_mark.astype(np.int64))
    # the forced cases are really there
    assert z[0, 1] == z[0, 3] == masked[0].max() and a[0, 0] == 1  # an exact tie: the lower index wins
    assert z[0, 5] == 0.0 and mk[0, 5] and a[0, 1] == 0  # a mark logit of exactly 0 does not mark
    if M > 1:
        assert a[1, 0] == 2
    if M > 2:
        assert a[2, 1] == 0 and a[3, 0] == 4 and np.isnan(lp[3]) and not legal[3]
        tie = (z[:, 1] == z[:, 3]) & (masked.max(1) == z[:, 1]) & mk[:, 1] & mk[:, 3]
        assert tie.sum() >= 2 and (a[tie, 0] == 1).all()
    # log-probs against fp64 log-softmax / log-sigmoid of the same logits
    z64 = z.astype(np.float64)
    m64 = np.where(mk[:, :5], z64[:, :5], -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = m64.max(1, keepdims=True)
        lsm = m64 - mx - np.log(np.exp(m64 - mx).sum(1, keepdims=True))
        ref = lsm[np.arange(M), a[:, 0]]
        logsig = -np.logaddexp(0, -z64[:, 5])  # log sigmoid(z)
        ref = ref + np.where(mk[:, 5], np.where(a[:, 1] == 1, logsig, logsig - z64[:, 5]), 0.0)
    ref[~legal] = np.nan
    err = np.abs(lp[legal] - ref[legal])
    print(f"  logp max abs err {err.max() if err.size else 0:.3g}")
    np.testing.assert_allclose(lp[legal], ref[legal], rtol=RTOL, atol=ATOL)
    assert np.isnan(lp[~legal]).all()
    # joint = the sum of the maze's two rows; the last row of an odd M alone
    lp2 = np.concatenate([lp, np.zeros(M % 2, np.float32)]).reshape(-1, 2)
    assert np.array_equal(jl, (lp2[:, 0] + lp2[:, 1]).astype(np.float32), equal_nan=True)
    # the logits-input form takes the same actions
    a2, lp_2, jl2 = ops.act(ref_logits[:, :5], ref_logits[:, 5], dmk, mode="greedy")
    assert np.array_equal(a2.cpu().numpy(), a)
    lp_2, jl2 = lp_2.cpu().numpy(), jl2.cpu().numpy()
    np.testing.assert_allclose(lp_2[legal], ref[legal], rtol=RTOL, atol=ATOL)
    assert np.isnan(lp_2[~legal]).all()
    lp2 = np.concatenate([lp_2, np.zeros(M % 2, np.float32)]).reshape(-1, 2)
    assert np.array_equal(jl2, (lp2[:, 0] + lp2[:, 1]).astype(np.float32), equal_nan=True)


def _pinned(fx, M, K, name, got):
    """`got` against the recorded array (tests/golden/record_sampler.py): bitwise, NaN (the no-legal-move row)
    equal to NaN; for a DIGEST_ONLY shape against the recorded SHA-256 of its bytes."""
    want = fx[f"{M}x{K}/{name}"]
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    if (M, K) in DIGEST_ONLY:
        return np.array_equal(np.frombuffer(hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest(), np.uint8),
                              want)
    return got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


@pytest.mark.parametrize("M,K", SHAPES)
def test_sample_mode_is_the_old_sampler(golden, M, K):
    """The plain form (ops.head_sample, ops.sample) and the mode form (ops.head_act, ops.act with mode="sample")
    both give what the sampler gave before the two were one kernel: tests/golden/sampler_pinned.npz."""
    fx = golden("sampler_pinned")
    if (M, K) in DIGEST_ONLY:  # the inputs are not in the file: rebuilt, and checked against their digests
        h, w, b, mk = _head_inputs(M, K)
        mk = mk.astype(np.uint8)
        assert all(_pinned(fx, M, K, n, x) for n, x in (("h", h), ("w", w), ("b", b), ("mk", mk))), \
            "_head_inputs no longer builds the recorded inputs (numpy's generator?): re-record"
    else:
        h, w, b, mk = (fx[f"{M}x{K}/{n}"] for n in ("h", "w", "b", "mk"))
    dh, dw, db, dmk = (torch.as_tensor(x).cuda() for x in (h, w, b, mk))
    off_dev = torch.tensor([3], dtype=torch.int64, device="cuda")
    for tag, od in (("hs", None), ("hsd", off_dev)):
        lg0 = torch.full((M, 6), float("nan"), device="cuda")
        lg1 = torch.full((M, 6), float("nan"), device="cuda")
        r0 = ops.head_sample(dh, dw, db, dmk, 11, 5, logits=lg0, offset_dev=od)
        r1 = ops.head_act(dh, dw, db, dmk, mode="sample", seed=11, offset=5, logits=lg1, offset_dev=od)
        for r, lg in ((r0, lg0), (r1, lg1)):
            assert _pinned(fx, M, K, "hs_logits", lg)
            for n, x in zip(("a", "lp", "jl"), r):
                assert _pinned(fx, M, K, f"{tag}_{n}", x), (tag, n)
    # and the logits-input pair, on those logits
    s0 = ops.sample(lg0[:, :5], lg0[:, 5], dmk, 11, 5)
    s1 = ops.act(lg0[:, :5], lg0[:, 5], dmk, mode="sample", seed=11, offset=5)
    for s in (s0, s1):
        for n, x in zip(("a", "lp", "jl"), s):
            assert _pinned(fx, M, K, f"s_{n}", x), n
    if M > 2:  # the forced rows are there: the no-legal-move row is NaN, and the device offset moved the draws
        assert np.isnan(s0[1].cpu().numpy()[3]) and not torch.equal(r0[0], s0[0])


# ---------------------------------------------------------------------------
# 3: the totals
# ---------------------------------------------------------------------------
def _ref_words(episodes):
    """episodes: (len, shortest, solved) in any order -> the 32 words (python ints)."""
    w = [0] * _lib.EVAL_WORDS
    w[_lib.EV_MIN_LEN_SOLVED] = 2**64 - 1
    for ln, sh, solved in episodes:
        w[_lib.EV_EPISODES] += 1
        w[_lib.EV_SUM_LEN] += ln
        if not solved:
            w[_lib.EV_TIMEOUTS] += 1
            continue
        w[_lib.EV_SOLVED] += 1
        w[_lib.EV_SUM_LEN_SOLVED] += ln
        w[_lib.EV_SUM_SHORT_SOLVED] += sh
        w[_lib.EV_MIN_LEN_SOLVED] = min(w[_lib.EV_MIN_LEN_SOLVED], ln)
        w[_lib.EV_MAX_LEN_SOLVED] = max(w[_lib.EV_MAX_LEN_SOLVED], ln)
        if sh <= 0:
            w[_lib.EV_BAD_SHORT] += 1
            continue
        w[_lib.EV_SUM_RATIO_Q16] += ln * 65536 // sh
        w[_lib.EV_HIST0 + min(max(4 * ln // sh - 4, 0), 15)] += 1
    return w


def _ref_result(w):
    """The result dict from the words, written out independently of marlmaze.evaluate."""
    ep, so, bad = w[0], w[1], w[9]
    return dict(episodes=ep, solved=so, timeouts=w[2], success_rate=so / ep if ep else None,
                mean_len=w[3] / ep if ep else None, mean_len_solved=w[4] / so if so else None,
                mean_shortest_solved=w[5] / so if so else None,
                mean_ratio=(w[8] / 65536.0) / (so - bad) if so - bad else None,
                min_len_solved=w[6] if so else None, max_len_solved=w[7] if so else None,
                ratio_hist=list(w[16:32]), ratio_bin_edges=[1.0 + 0.25 * k for k in range(16)], bad_shortest=bad)


def _streams(n, T=50):
    rng = np.random.default_rng(n)
    cls = (np.arange(n) + 1) % 4  # 0: never finishes; 1: finishes often (more than any quota here); 2, 3: sometimes
    p = np.choose(cls, [0.0, 0.3, 0.04, 0.1])
    done = (rng.random((T, n)) < p).astype(np.uint8)
    solved = rng.random((T, n)) < 0.6
    reward = np.where(solved, 1.0, rng.choice([0.0, 0.5], (T, n))).astype(np.float32)  # 1.0 also where not done
    stats = np.stack([rng.integers(1, 200, (T, n)), rng.integers(0, 40, (T, n))], -1).astype(np.int32)
    # fixed cases, each the FIRST episode of its maze: a ratio below 1, one above 4.75, shortest == 0, a timeout
    for m, (ln, sh, rw) in {0: (3, 10, 1.0), 1: (200, 5, 1.0), 4: (7, 0, 1.0), 5: (60, 9, 0.0)}.items():
        if m < n:
            done[0, m], reward[0, m], stats[0, m] = 1, rw, (ln, sh)
    return done, reward, stats


@pytest.mark.parametrize("quota", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_totals_equal_numpy(n, quota):
    done, reward, stats = _streams(n)
    T = done.shape[0]
    counted = np.zeros(n, np.int64)
    eps = []
    for t in range(T):
        for m in np.nonzero(done[t])[0]:
            if counted[m] < quota:
                counted[m] += 1
                eps.append((int(stats[t, m, 0]), int(stats[t, m, 1]), reward[t, m] == np.float32(1.0)))
    want = _ref_words(eps)
    if n >= 63:  # the stream holds what it should
        assert (done.sum(0) > quota).any() and (done.sum(0) == 0).any() and want[_lib.EV_TIMEOUTS] > 0
        assert want[_lib.EV_BAD_SHORT] > 0 and want[_lib.EV_HIST0] > 0 and want[_lib.EV_HIST0 + 15] > 0
    d_done, d_rew, d_st = (torch.as_tensor(x).cuda() for x in (done, reward, stats))
    tot = EvalTotals(n, quota)
    got = []
    for _ in range(2):
        tot.init()
        for t in range(T):
            tot.accum(d_done[t], d_rew[t], d_st[t])
        got.append((tot.words(), tot.counted.cpu().numpy().astype(np.int64)))
    print(f"n={n} quota={quota}: episodes {got[0][0][0]} (want {want[0]}), solved {got[0][0][1]} (want {want[1]})")
    assert got[0][0] == want
    assert np.array_equal(got[0][1], counted)
    assert got[1][0] == got[0][0] and np.array_equal(got[1][1], got[0][1])  # the same again
    assert tot.read() == _ref_result(want)


# ---------------------------------------------------------------------------
# 4: PPO.evaluate replayed on the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("greedy", [True, False])
def test_evaluate_replayed_on_oracle(golden, greedy):
    """The CPU oracle run of this configuration (greedy) gave 54 solved and 74 timed out in 120 steps."""
    n, E = 64, 2
    cfg = dict(default_size=(6, 6), max_timestep=60)
    ag = _agent(n_envs=n)
    _load(ag, golden("ckpt_logits"))
    res, rec = ag.evaluate(episodes_per_env=E, greedy=greedy, n_envs=n, env_config=cfg, seed_base=0, record=True)
    acts, done, rew = (rec[k].cpu().numpy() for k in ("actions", "done", "reward"))
    T = acts.shape[0]
    assert acts.shape == (T, n, 2, 2) and done.shape == (T, n) and rew.shape == (T, n)
    ora = OracleEnv(n, seeds=np.arange(n, dtype=np.uint64), **cfg)
    ora.reset_all()
    steps = np.zeros(n, np.int64)
    counted = np.zeros(n, np.int64)
    eps = []
    for t in range(T):
        shortest = [ora.maze(i)["path_len"] for i in range(n)]
        _, _, orw, od = ora.step_all(acts[t], auto_reset=True)
        assert np.array_equal(done[t].astype(bool), od), t
        assert np.array_equal(rew[t], orw), t
        steps += 1
        for m in np.nonzero(od)[0]:
            if counted[m] < E:
                counted[m] += 1
                eps.append((int(steps[m]), int(shortest[m]), orw[m] == np.float32(1.0)))
            steps[m] = 0
    want = _ref_result(_ref_words(eps))
    print(f"greedy={greedy}: T={T} solved {res['solved']} timeouts {res['timeouts']} mean_ratio {res['mean_ratio']}")
    assert res["env_steps"] == n * T and T <= E * cfg["max_timestep"]
    seconds = res.pop("seconds")
    assert seconds > 0 and res.pop("env_steps") == n * T
    assert res == want
    assert res["episodes"] == n * E
    if greedy:
        assert res["solved"] >= 1 and res["timeouts"] >= 1


# ---------------------------------------------------------------------------
# 5, 6: invisible to training; reproducible
# ---------------------------------------------------------------------------
def test_evaluation_is_invisible_to_training():
    def make():
        return _agent(n_envs=64, horizon=4, sample_seed=5,
                      env_config=dict(default_size=(10, 10), max_timestep=60, seed_base=0))

    a, b = make(), make()
    for ag in (a, b):
        ag.rollout()
        ag._carry_over()  # as get_batch does between rollouts: the second rollout continues the episodes
    state, off, armed, prec = random.getstate(), a._sample_offset, a._flag_armed, a.actor.gemm_prec
    venv, bufs = a.venv, a._bufs
    cpu_rng, gpu_rng = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    res = a.evaluate(n_envs=32, env_config=dict(default_size=(6, 6), max_timestep=20))
    assert res["episodes"] == 32
    assert random.getstate() == state and a._sample_offset == off and a._flag_armed == armed
    assert a.venv is venv and a._bufs is bufs and a.actor.gemm_prec == prec
    assert torch.equal(torch.random.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    ba, bb = a.rollout(), b.rollout()
    for k in ba:
        x, y = ba[k].cpu().numpy(), bb[k].cpu().numpy()
        assert x.tobytes() == y.tobytes(), k  # bitwise
    assert a._sample_offset == b._sample_offset


def test_greedy_evaluation_is_reproducible(golden):
    c = golden("ckpt_logits")
    ag = _agent(n_envs=64)
    _load(ag, c)
    kw = dict(n_envs=48, env_config=dict(default_size=(6, 6), max_timestep=30), seed_base=7)
    r0, r1 = ag.evaluate(**kw), ag.evaluate(**kw)
    r0.pop("seconds"), r1.pop("seconds")
    assert r0 == r1 and r0["episodes"] == 48
    # the single-sample API: the most likely legal move, a mark where its logit is > 0
    obs = c["obs"].reshape(-1, 65)[0]
    mask = [1, 1, 0, 1, 1, 1]
    with torch.no_grad():
        ml, kl = ag.actor(torch.as_tensor(obs).cuda().view(1, 65))
    ml, kl = ml.cpu().numpy()[0], float(kl.cpu().numpy().reshape(-1)[0])
    ml[2] = -np.inf
    off = ag._sample_offset
    (move, mark), lp = ag.get_action(obs, mask, greedy=True)
    assert move == int(np.argmax(ml)) and mark == int(kl > 0) and ag._sample_offset == off
    assert lp.shape == (1, 1) and torch.isfinite(lp).all()
    assert ag.get_action(obs, mask, greedy=True)[0] == [move, mark]


# ---------------------------------------------------------------------------
# 7: DP
# ---------------------------------------------------------------------------
_WORKER = r"""
import json, os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
rank = int(sys.argv[1])
os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                  MASTER_PORT=sys.argv[2])
from marlmaze.dist import DP
from marlmaze.PPO import PPO
import torch.distributed as dist
dp = DP.from_env(backend="gloo")
assert dp.rank == rank and dp.world == 2
ag = PPO(2, n_envs=32, dp=dp, load=False, verbose=False, save=False, sample_seed=21)
fx = np.load({ckpt!r})  # the shipped checkpoint's weights: some episodes are solved, some time out
ag.actor.load_state_dict({{k[6:]: torch.as_tensor(fx[k]) for k in fx.files if k.startswith("actor/")}})
res = ag.evaluate(greedy=True, n_envs=32, env_config=dict(default_size=(6, 6), max_timestep=40), seed_base=0)
json.dump(res, open(sys.argv[3] + "_%d.json" % rank, "w"))
dist.destroy_process_group()
"""


def test_two_rank_evaluation_equals_one_process(tmp_path, golden):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd"), repo=REPO,
                                     ckpt=os.path.join(REPO, "tests", "golden", "ckpt_logits.npz")))
    out = str(tmp_path / "rank")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    procs = [subprocess.Popen([sys.executable, "-u", str(script), str(r), port, out], env=dict(os.environ))
             for r in range(2)]
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0, 0], rcs
    r = [json.load(open(f"{out}_{k}.json")) for k in range(2)]
    ag = _agent(n_envs=64, sample_seed=21)
    _load(ag, golden("ckpt_logits"))
    one = ag.evaluate(greedy=True, n_envs=64, seed_base=0, env_config=dict(default_size=(6, 6), max_timestep=40))
    for d in r + [one]:
        d.pop("seconds")
    print(f"one process: {one['episodes']} episodes, {one['solved']} solved; two ranks: {r[0]['solved']} solved")
    assert r[0] == r[1] == one and one["episodes"] == 64
    assert one["solved"] >= 1 and one["timeouts"] >= 1  # the sums, the min and the max all carry something


# ---------------------------------------------------------------------------
# 8: the command line
# ---------------------------------------------------------------------------
def test_cli_in_process(tmp_path, capsys):
    from marlmaze import evaluate

    path = str(tmp_path / "PPO.pth")
    _agent(n_envs=32, model_path=path).save_parameters()
    ret = evaluate.main(["--model", path, "--n-envs", "32", "--size", "6", "--max-timestep", "20", "--episodes", "1",
                         "--json"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["episodes"] == 32 and res["solved"] + res["timeouts"] == 32 and res["mode"] == "greedy"
    assert res["env_steps"] == ret["env_steps"] and len(res["ratio_hist"]) == 16


# ---------------------------------------------------------------------------
# the optional hooks: train(eval_every), display_policy(greedy=True)
# ---------------------------------------------------------------------------
def test_train_eval_every():
    ag = _agent(n_envs=64, horizon=5, epochs=2, batch_size=320, sample_seed=3,
                env_config=dict(default_size=(6, 6), max_timestep=30, seed_base=0))
    ag.train(eval_every=2, eval_kwargs=dict(n_envs=32, env_config=dict(default_size=(6, 6), max_timestep=20)))
    assert len(ag.history) == 2 and "eval" not in ag.history[0]
    ev = ag.history[1]["eval"]
    assert ev["episodes"] == 32 and ev["solved"] + ev["timeouts"] == 32
    plain = _agent(n_envs=64, horizon=5, epochs=1, batch_size=320, sample_seed=3,
                   env_config=dict(default_size=(6, 6), max_timestep=30, seed_base=0))
    plain.train()  # the default: today's history entries
    assert "eval" not in plain.history[0] and set(plain.history[0]) == set(ag.history[0])


def test_display_policy_greedy_is_deterministic():
    from marlmaze.maze import Maze
    from marlmaze.maze_agent import Agent

    def frames():
        brain = _agent(n_envs=16, sample_seed=6)
        agents = (Agent("RED", brain, "red", "palevioletred1", 2), Agent("BLUE", brain, "royalblue1", "darkslategray1", 3))
        maze = Maze(agents=agents, max_timestep=1200, default_size=[4, 4])
        random.seed(5)
        out = maze.display_policy(steps=4, greedy=True)
        return brain._sample_offset, [np.asarray(f) for f in out]

    (off0, f0), (off1, f1) = frames(), frames()
    assert off0 == off1 == 0  # no draw was made
    assert len(f0) == len(f1) >= 5 and all(np.array_equal(x, y) for x, y in zip(f0, f1))


# ---------------------------------------------------------------------------
# the range guard inside evaluate: repeated at x3, collectively under DP
# ---------------------------------------------------------------------------
_EV_CFG = dict(n_envs=32, env_config=dict(default_size=(6, 6), max_timestep=20))


def _flag():
    from marlmaze import x3

    return int(x3.range_flag(clear=False))


def _out_of_range(agent):
    """Layer 0 scaled by 2^20: the next layer's activations leave the fp16 planes' range (|x| >= 2^15), fp32
    holds them easily."""
    with torch.no_grad():
        agent.actor.layers[0].weight.mul_(2.0 ** 20)
        agent.actor.layers[0].bias.mul_(2.0 ** 20)


def test_evaluate_repeats_at_x3_and_restores_the_flag():
    from marlmaze import x3

    ag = _agent(n_envs=32)
    prec = ag.actor.gemm_prec
    assert prec != "x3"
    _out_of_range(ag)
    try:
        x3.range_flag(clear=True)
        with pytest.warns(UserWarning, match="repeated at x3"):
            res = ag.evaluate(**_EV_CFG)
        assert _flag() == 0 and ag.actor.gemm_prec == prec  # the flag as it was found, the precision restored
        assert res["episodes"] == 32 and res["solved"] + res["timeouts"] == 32
        ag.actor.gemm_prec = "x3"  # the same evaluation at x3 from the start
        want = ag.evaluate(**_EV_CFG)
        ag.actor.gemm_prec = prec
        res.pop("seconds"), want.pop("seconds")
        assert res == want
        # a flag that is already raised (the rollout's) stays raised, and the run uses x3 without a repeat
        with torch.no_grad():
            ag.actor(torch.ones(64, 65, device="cuda") * 2.0 ** 17)
        assert _flag() == 1
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            again = ag.evaluate(**_EV_CFG)
        assert not [w for w in caught if "repeated at x3" in str(w.message)]
        again.pop("seconds")
        assert again == want and _flag() == 1 and ag.actor.gemm_prec == prec
    finally:
        x3.range_flag(clear=True)


_RANGE_WORKER = r"""
import json, os, sys, warnings
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import torch
rank = int(sys.argv[1])
os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                  MASTER_PORT=sys.argv[2])
from marlmaze import x3
from marlmaze.dist import DP
from marlmaze.PPO import PPO
import torch.distributed as dist
dp = DP.from_env(backend="gloo")
ag = PPO(2, n_envs=32, dp=dp, load=False, verbose=False, save=False, sample_seed=21)
prec = ag.actor.gemm_prec
cfg = dict(n_envs=32, env_config=dict(default_size=(6, 6), max_timestep=20))
out = dict(prec=prec)
# A: the flag is already raised on rank 1 only: both ranks run at x3, nobody repeats, the flags stay
if rank == 1:
    with torch.no_grad():
        ag.actor(torch.ones(64, 65, device="cuda") * 2.0 ** 17)
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    out["A"] = ag.evaluate(**cfg)
out["A_warned"] = sum("repeated at x3" in str(x.message) for x in w)
out["A_flag"] = int(x3.range_flag(clear=True))
# B: only rank 1's weights leave the range during the run: both ranks repeat at x3
if rank == 1:
    with torch.no_grad():
        ag.actor.layers[0].weight.mul_(2.0 ** 20)
        ag.actor.layers[0].bias.mul_(2.0 ** 20)
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    out["B"] = ag.evaluate(**cfg)
out["B_warned"] = sum("repeated at x3" in str(x.message) for x in w)
out["B_flag"] = int(x3.range_flag(clear=True))
out["prec_after"] = ag.actor.gemm_prec
json.dump(out, open(sys.argv[3] + "_%d.json" % rank, "w"))
dist.destroy_process_group()
"""


def test_evaluate_range_guard_is_collective_under_dp(tmp_path):
    """One rank's range flag takes BOTH ranks down the same branch (the same collectives: no rank is left waiting
    in another one's all-reduce)."""
    script = tmp_path / "worker.py"
    script.write_text(_RANGE_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd"), repo=REPO))
    out = str(tmp_path / "rank")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    procs = [subprocess.Popen([sys.executable, "-u", str(script), str(r), port, out], env=dict(os.environ))
             for r in range(2)]
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0, 0], rcs
    r = [json.load(open(f"{out}_{k}.json")) for k in range(2)]
    for k in range(2):
        for ph in ("A", "B"):
            r[k][ph].pop("seconds")
        assert r[k]["prec_after"] == r[k]["prec"] != "x3"
        assert r[k]["A"]["episodes"] == r[k]["B"]["episodes"] == 64
    assert r[0]["A"] == r[1]["A"] and r[0]["B"] == r[1]["B"]  # global totals on both ranks
    assert [r[k]["A_warned"] for k in range(2)] == [0, 0] and [r[k]["A_flag"] for k in range(2)] == [0, 1]
    assert [r[k]["B_warned"] for k in range(2)] == [1, 1] and [r[k]["B_flag"] for k in range(2)] == [0, 0]
    # phase A is the x3 evaluation of the common weights: one process at x3 gives the same totals
    ag = _agent(n_envs=64, sample_seed=21)
    ag.actor.gemm_prec = "x3"
    one = ag.evaluate(n_envs=64, env_config=dict(default_size=(6, 6), max_timestep=20))
    one.pop("seconds")
    assert one == r[0]["A"]
