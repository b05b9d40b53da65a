"""CPU-only checks of the host side: the C ABI library loads and exports every
declared symbol, the struct mirrors match the header, the product networks
initialise exactly like the reference, and the data-parallel update logic
(gloo, world size 2) equals a single-process update on the union batch."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from marlmaze import _lib
from marlmaze.vecmaze import AGENT_DTYPE, MAZE_DTYPE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "marlmaze.h")


def _ensure_lib():
    if not os.path.exists(_lib.LIB_PATH):
        from marlmaze import _build
        _build.build()


def test_library_exports_every_declared_symbol():
    _ensure_lib()
    decl = set(re.findall(r"^\s*(?:int|long)\s+(mm_\w+)\s*\(", open(HEADER).read(), re.M))
    assert decl == set(_lib.EXPORTS), decl ^ set(_lib.EXPORTS)
    L = _lib.lib()
    for sym in decl:
        assert getattr(L, sym) is not None
    assert L.mm_version() >= 100
    assert L.mm_layout_stride(10, 10, 0, 6, 12) == 19 * 19
    assert L.mm_layout_stride(4, 4, 1, 12, 13) == 25 * 25
    assert L.mm_layout_stride(30, 30, 0, 6, 12) < 0  # beyond MM_MAX_SIDE
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for sym in decl:
        assert re.search(rf"\bT {sym}\b", nm), sym


def test_struct_mirrors_match_header():
    h = open(HEADER).read()
    assert "int32_t spawn1;" in h and AGENT_DTYPE.itemsize == 32 and MAZE_DTYPE.itemsize == 32
    # every field offset and the size of mm_env_t as the C compiler lays it out
    import subprocess
    import tempfile
    fields = [f for f, _ in _lib.EnvDesc._fields_]
    prog = ("#include <stddef.h>\n#include <stdio.h>\n#include \"marlmaze.h\"\nint main(void){printf(\"%zu\\n\", "
            "sizeof(mm_env_t));" + "".join(f'printf("%zu\\n", offsetof(mm_env_t, {f}));' for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "m.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", os.path.join(d, "m"), os.path.join(d, "m.c")],
                       check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "m")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    assert out[0] == ctypes_size(_lib.EnvDesc)
    assert out[1:] == [getattr(_lib.EnvDesc, f).offset for f in fields]
    for name, val in (("MM_OBS_DIM", _lib.OBS_DIM), ("MM_MASK_DIM", _lib.MASK_DIM),
                      ("MM_RNG_WORDS", _lib.RNG_WORDS), ("MM_MAX_SIDE", _lib.MAX_SIDE)):
        assert re.search(rf"#define {name} {val}\b", h), name


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_product_networks_initialise_like_reference(golden):
    from marlmaze.networks import Actor, Critic

    n = golden("nets")
    old = torch.get_num_threads()
    torch.set_num_threads(4)  # orthogonal_ (LAPACK QR) depends on the thread count
    try:
        torch.manual_seed(3234)
        actor, critic = Actor([264, 264, 264]), Critic(2, hidden_sizes=[64, 64])
    finally:
        torch.set_num_threads(old)
    sd = actor.state_dict()
    assert len(sd) == 59 and len(critic.state_dict()) == 6
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), n["actor/" + k]), k
    for k, v in critic.state_dict().items():
        assert np.array_equal(v.numpy(), n["critic/" + k]), k
    # packed-GEMM forward == reference arithmetic (CPU, tight tolerance)
    o = torch.as_tensor(n["obs"])
    with torch.no_grad():
        mv, mr = actor(o.reshape(-1, 65))
        v = critic(o)
    np.testing.assert_allclose(mv.numpy(), n["move_logits"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mr.numpy(), n["mark_logits"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v.numpy(), n["values"], rtol=1e-5, atol=1e-6)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_DP_WORKER = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
import torch.distributed as dist
from marlmaze.dist import DP
from marlmaze.PPO import PPO
rank, world = int(sys.argv[1]), int(sys.argv[5])
os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
dp = DP.from_env(backend="gloo")
torch.set_num_threads(1)
data = np.load(sys.argv[3])
Bl = data["obs"].shape[0] // world
sl = slice(rank * Bl, (rank + 1) * Bl)
ag = PPO(2, batch_size=world * Bl - (world * Bl) % (5 * world), lr=1e-6, device="cpu", dp=dp, load=False,
         verbose=False, save=False)
hist = ag.update(*(torch.as_tensor(data[k][sl]) for k in ("obs", "act", "logp", "masks", "adv", "val")),
                 index_list=data["idx%d" % rank])
out = dict(hist=hist.numpy(), **{{k: v.numpy() for k, v in ag.actor.state_dict().items()}},
           **{{"critic." + k: v.numpy() for k, v in ag.critic.state_dict().items()}})
np.savez(sys.argv[4] + "_%d.npz" % rank, **out)
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world", [2, 4, 8])
def test_data_parallel_update_equals_single_process(tmp_path, golden, world):
    """``world`` gloo ranks, each with 1/world of the batch and its own shuffle,
    give the same losses and parameters as one process whose minibatches are
    the unions (results independent of the world size), and
    every rank ends with the same parameters bit for bit."""
    from marlmaze.PPO import PPO

    t = golden("train_small")
    B = 640
    rng = np.random.default_rng(world)
    data = dict(obs=t["obs"][:B], act=t["actions"][:B], logp=t["logp"][:B], masks=t["masks"][:B],
                adv=t["advs"][:B], val=t["vals"][:B])
    Bl = B // world
    idx = [rng.permutation(Bl) for _ in range(world)]
    fx = str(tmp_path / "dp_in.npz")
    np.savez(fx, **{f"idx{r}": idx[r] for r in range(world)}, **data)
    port = str(_free_port())
    out = str(tmp_path / "dp_out")
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_DP_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd"), repo=REPO))
    procs = [subprocess.Popen([sys.executable, script, str(r), port, fx, out, str(world)]) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    got = [np.load(out + f"_{r}.npz") for r in range(world)]
    for r in range(1, world):  # parameters identical on every rank
        for k in got[0].files:
            if k != "hist":
                assert np.array_equal(got[r][k], got[0][k]), (r, k)
    # single process: minibatch k = the union over ranks of slice k
    local_bs = Bl - Bl % 5
    mb_l = local_bs // 5
    glob = []
    for k in range(5):
        for r in range(world):
            glob += list(r * Bl + idx[r][k * mb_l:(k + 1) * mb_l])
    torch.set_num_threads(1)
    ag = PPO(2, batch_size=world * local_bs, lr=1e-6, device="cpu", load=False, verbose=False, save=False)
    hist = ag.update(*(torch.as_tensor(data[k]) for k in ("obs", "act", "logp", "masks", "adv", "val")),
                     index_list=np.asarray(glob))
    np.testing.assert_allclose(got[0]["hist"][:, :2], hist.numpy()[:, :2], rtol=1e-5, atol=1e-6)
    for k, v in ag.actor.state_dict().items():
        np.testing.assert_allclose(got[0][k], v.numpy(), rtol=0, atol=3e-6)
    for k, v in ag.critic.state_dict().items():
        np.testing.assert_allclose(got[0]["critic." + k], v.numpy(), rtol=0, atol=3e-6)


def test_integration_struct_matches_header():
    """INTEGRATION.md section 2's ctypes mirror of mm_env_t has the header's 19
    fields at the header's offsets (the binding a maintainer copies must not be
    shorter than the struct the library reads), and the library reports the
    same size (mm_env_desc_size) and ABI major version."""
    import ctypes

    _ensure_lib()
    md = open(os.path.join(REPO, "INTEGRATION.md")).read()
    block = re.search(r"```python\n(import ctypes, torch.*?)```", md, re.S).group(1)
    cls = re.search(r"(class mm_env_t\(ctypes\.Structure\):.*?\])\n\n", block, re.S).group(1)
    ns = {"ctypes": ctypes}
    exec(cls, ns)
    T = ns["mm_env_t"]
    names = [f for f, _ in T._fields_]
    assert len(names) == 19 and names == [f for f, _ in _lib.EnvDesc._fields_]
    assert [getattr(T, f).offset for f in names] == [getattr(_lib.EnvDesc, f).offset for f in names]
    L = _lib.lib()
    assert ctypes.sizeof(T) == L.mm_env_desc_size() == ctypes.sizeof(_lib.EnvDesc)
    assert L.mm_version() // 100 == _lib.VERSION // 100 == 3
    assert "mm_env_desc_size() == ctypes.sizeof(mm_env_t)" in block


_FLAG_WORKER = r"""
import os, sys
sys.path.insert(0, {pkg!r})
import torch
import torch.distributed as dist
from marlmaze.dist import DP
rank, world = int(sys.argv[1]), int(sys.argv[3])
os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
dp = DP.from_env(backend="gloo")
out = []
for pre_rank, post_rank in ((None, world - 1), (0, None), (None, None), (1, 1)):
    pre = torch.tensor([int(rank == pre_rank)], dtype=torch.int32)
    post = torch.tensor([int(rank == post_rank)], dtype=torch.int32)
    out.append(dp.raised_on_any_rank(pre, post))
print("FLAGS", rank, out, flush=True)
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world", [2, 4])
def test_range_guard_flags_are_collective(tmp_path, world):
    """DP.raised_on_any_rank (the x2 range guard's decision): a flag raised on ONE rank is seen by every rank (MAX
    all-reduce before the host read), so all ranks redo / discard together and issue the same collectives."""
    script = str(tmp_path / "flags.py")
    open(script, "w").write(_FLAG_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd")))
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, script, str(r), port, str(world)], stdout=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert [p.returncode for p in procs] == [0] * world
    want = "[(0, 1), (1, 0), (0, 0), (1, 1)]"
    for r, o in enumerate(outs):
        assert f"FLAGS {r} {want}" in o, o


_WORDS_WORKER = r"""
import json, os, sys
sys.path.insert(0, {pkg!r})
import torch
import torch.distributed as dist
from marlmaze import _lib
from marlmaze.dist import DP
from marlmaze.evaluate import NONE_MIN, reduce_words
rank = int(sys.argv[1])
os.environ.update(RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])


class CountingDP(DP):  # the collectives that reduce_words issues
    calls = 0

    def allreduce_sum(self, t):
        self.calls += 1
        return super().allreduce_sum(t)

    def allreduce_max(self, t):
        self.calls += 1
        return super().allreduce_max(t)


base = DP.from_env(backend="gloo")
dp = CountingDP(base.rank, base.world)


def ev(episodes, solved, sum_len, sum_len_solved, mn, mx, hist):
    w = [0] * _lib.EVAL_WORDS
    w[_lib.EV_EPISODES], w[_lib.EV_SOLVED], w[_lib.EV_TIMEOUTS] = episodes, solved, episodes - solved
    w[_lib.EV_SUM_LEN], w[_lib.EV_SUM_LEN_SOLVED] = sum_len, sum_len_solved
    w[_lib.EV_MIN_LEN_SOLVED], w[_lib.EV_MAX_LEN_SOLVED] = mn, mx
    for b, c in hist.items():
        w[_lib.EV_HIST0 + b] = c
    return w


def pw(rated, excess, hist):
    w = [0] * _lib.PAR_WORDS
    w[_lib.PAR_EPISODES], w[_lib.PAR_SUM_LEN], w[_lib.PAR_MAX_EXCESS] = rated, 10 * rated + rank, excess
    for b, c in hist.items():
        w[_lib.PAR_HIST0 + b] = c
    return w


nothing = ev(2, 0, 40, 0, NONE_MIN, 0, {{}})  # two timed-out episodes: the min word as mm_eval_init left it
some = ev(3, 2, 36, 16, 7, 9, {{0: 1, 15: 1}})
out = []
for mine, par in (((nothing, some)[rank], None),                                   # 1, 4: one rank has nothing
                  (nothing, None),                                                 # 2: neither has
                  (some, pw(2 + rank, (3, 11)[rank], {{rank: 1, 5: 1 + rank}}))):      # 3: with par
    before = dp.calls
    w, p = reduce_words(list(mine), None if par is None else list(par), dp, torch.device("cpu"))
    out.append(dict(words=w, pwords=p, calls=dp.calls - before))
single = reduce_words(some, None, DP.single(), torch.device("cpu"))
out.append(dict(same=single[0] is some and single[1] is None))
print("WORDS", rank, json.dumps(out), flush=True)
dist.destroy_process_group()
"""


def test_evaluation_words_reduce_across_ranks(tmp_path):
    """marlmaze.evaluate.reduce_words on two gloo ranks: the sums add, the max word is the larger one and the min
    word the smaller one, where a rank that solved nothing (min word NONE_MIN, max word 0) leaves the other rank's
    extremes alone and two such ranks give NONE_MIN again; without par words no par collective is issued; under
    DP.single() the input comes back as it is."""
    import json

    from marlmaze.evaluate import NONE_MIN, result_from_par_words, result_from_words

    script = str(tmp_path / "words.py")
    open(script, "w").write(_WORDS_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd")))
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, script, str(r), port], stdout=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0]
    got = [json.loads(re.search(rf"^WORDS {r} (.*)$", o, re.M).group(1)) for r, o in enumerate(outs)]
    assert got[0] == got[1]  # every rank reads the same words
    one, neither, with_par, single = got[0]
    # 1: rank 0 solved nothing, rank 1 has min 7 and max 9
    w = one["words"]
    assert (w[_lib.EV_MIN_LEN_SOLVED], w[_lib.EV_MAX_LEN_SOLVED]) == (7, 9)
    assert (w[_lib.EV_EPISODES], w[_lib.EV_SOLVED], w[_lib.EV_TIMEOUTS]) == (5, 2, 3)
    assert (w[_lib.EV_SUM_LEN], w[_lib.EV_SUM_LEN_SOLVED]) == (76, 16)
    assert w[_lib.EV_HIST0:] == [1] + [0] * 14 + [1] and len(w) == _lib.EVAL_WORDS
    r = result_from_words(w)
    assert (r["min_len_solved"], r["max_len_solved"], r["episodes"]) == (7, 9, 5)
    # 4: no par words, no par collective: the two of the totals and nothing else (and nobody waited for more)
    assert one["pwords"] is None and one["calls"] == 2
    # 2: neither rank solved anything
    w = neither["words"]
    assert w[_lib.EV_MIN_LEN_SOLVED] == NONE_MIN and w[_lib.EV_MAX_LEN_SOLVED] == 0 and w[_lib.EV_EPISODES] == 4
    assert result_from_words(w)["min_len_solved"] is None and neither["calls"] == 2
    # 3: both solved (min 7 = 7, max 9 = 9, sums doubled); par's max word 3 and 11, its bins added
    w, p = with_par["words"], with_par["pwords"]
    assert (w[_lib.EV_MIN_LEN_SOLVED], w[_lib.EV_MAX_LEN_SOLVED], w[_lib.EV_EPISODES]) == (7, 9, 6)
    assert p[_lib.PAR_MAX_EXCESS] == 11 and p[_lib.PAR_EPISODES] == 5 and p[_lib.PAR_SUM_LEN] == 20 + 31
    hist = p[_lib.PAR_HIST0:]
    assert (hist[0], hist[1], hist[5]) == (1, 1, 3) and sum(hist) == 5 and len(p) == _lib.PAR_WORDS
    assert result_from_par_words(p)["max_excess"] == 11 and with_par["calls"] == 4
    # 5: DP.single()
    assert single == dict(same=True)


@pytest.mark.parametrize("world", [2])
def test_global_advantage_statistics(world):
    from marlmaze.dist import DP

    x = torch.randn(1000, dtype=torch.float32)
    m, s = DP.single().global_mean_std(x)
    assert torch.allclose(m, x.mean()) and torch.allclose(s, x.std())


def test_bench_dump_outputs_writes_fixed_float32_arrays(tmp_path):
    """bench.py --dump-outputs: every array is written as float32 under its name, small ones whole and
    large ones as the same seeded sample on every call (the indices depend on the size alone)."""
    import types

    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    T, n = 3, 5
    g = torch.Generator().manual_seed(0)
    big = bench.DUMP_MAX_ELEMS + 1001
    bufs = dict(obs=torch.rand(big, generator=g), masks=torch.randint(0, 2, (T + 1, n, 2, 6), dtype=torch.uint8),
                act=torch.randint(0, 5, (T, n, 2, 2), dtype=torch.int8), last_val=torch.rand(n, generator=g))
    for k in ("logp", "val", "rew", "adv", "rtg"):
        bufs[k] = torch.rand(T, n, generator=g)
    bufs["done"] = torch.randint(0, 2, (T, n), dtype=torch.uint8)
    agent = types.SimpleNamespace(_bufs=bufs, horizon=T, flat=types.SimpleNamespace(data=torch.rand(77, generator=g)))
    hist = torch.rand(25, 4, generator=g)
    out = [tmp_path / "a", tmp_path / "b"]
    for d in out:
        bench.dump_outputs(str(d), agent, hist)
    names = sorted(p.name for p in out[0].iterdir())
    assert names == sorted(k + ".npy" for k in list(bufs) + ["update_hist", "params"])
    total = 0
    for name in names:
        x, y = np.load(out[0] / name), np.load(out[1] / name)
        assert x.dtype == np.float32 and x.ndim == 1 and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64e6
    assert np.array_equal(np.load(out[0] / "act.npy"), bufs["act"].reshape(-1).float().numpy())
    assert np.array_equal(np.load(out[0] / "update_hist.npy"), hist.reshape(-1).numpy())
    obs = np.load(out[0] / "obs.npy")
    idx = np.random.default_rng(0).integers(0, big, size=bench.DUMP_MAX_ELEMS)
    assert np.array_equal(obs, bufs["obs"].numpy()[idx])


def test_bench_bounded_cpu_sample_reports_progress():
    """bench.py's os.cpu_count()-thread CPU leg (_cpu_epoch_bounded): a finished
    child extrapolates its rollout chunks and one update pass to the epoch; a
    child cut by the time limit before any chunk reports that instead of a rate."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from oracle.env import OracleEnv
    from oracle.ppo import CpuPPOPort

    port = CpuPPOPort(OracleEnv(1, default_size=(10, 10), max_timestep=1200, seeds=[0]), batch_size=15000)
    steps, batch = port.get_batch(max_steps=40)
    r = bench._cpu_epoch_bounded(1, (15600, batch), max_steps=20, timeout=120)
    assert r["timed_out_s"] is None and r["env_steps"] == 15600 and r["env_steps_per_s"] > 0
    assert r["rollout_env_steps_per_s"] > 0 and r["epoch_s"] > r["update_s"] > 0
    assert "first 20 rollout env-steps" in r["sampled"]
    cut = bench._cpu_epoch_bounded(1, (15600, batch), max_steps=20, timeout=0.01)
    assert cut["timed_out_s"] == 0.01 and cut["env_steps_per_s"] == 0.0
