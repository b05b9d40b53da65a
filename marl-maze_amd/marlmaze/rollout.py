"""Rollout collection for ``PPO`` (PPO.get_batch, PPO.py:89-152): the per-step buffers, one policy step, and
the three collectors built from it.  Every function takes the agent (a ``PPO``); ``PPO.rollout``,
``PPO.get_batch``, ``PPO._ensure_env`` and ``PPO._carry_over`` are calls of them.

* ``step_buffers``: the buffers one step reads and writes, for T steps of n mazes -- the agent's ``_bufs``
  (zeroed, ``horizon`` steps) and the episode batches' chunks (uninitialised).
* ``policy_step``: the critic's value of row t (the per-step form only), ``Actor.sample_actions`` into row t,
  ``env_step`` into row t + 1.
* ``fixed_horizon``: every maze advances ``horizon`` steps, the values of all steps in one critic launch after
  the loop (``BATCHED_CRITIC``), then the GAE.  ``captured`` is the same launches recorded once as a HIP graph and
  replayed (``Replay``).  ``episode_batch`` collects whole episodes only, as the reference does.

No host synchronisation inside a fixed-horizon rollout; one per chunk in an episode batch.
"""
import random

import numpy as np
import torch

from . import ops, x3
from .vecmaze import VecMaze

# the fixed-horizon rollout's critic values in ONE launch over all T (+1) steps' observations after the env loop
# (they depend on the observations only, and the weights do not change during a rollout): no critic launch per
# step.  False: one launch per step, before the step's actions (the reference form of the tests)
BATCHED_CRITIC = True


def step_buffers(T, n, device, zeroed):
    """The per-step buffer set for T steps of n mazes: row t of obs / masks is the state before step t (row T
    the state after the last one), row t of the others what step t produced.  ``val`` / ``last_val`` are views
    of ``val_all`` (the T values + the bootstrap row)."""
    new = torch.zeros if zeroed else torch.empty
    b = {k: new(shape, dtype=dtype, device=device) for k, shape, dtype in (
        ("obs", (T + 1, n, 2, 65), torch.float32), ("masks", (T + 1, n, 2, 6), torch.uint8),
        ("act", (T, n, 2, 2), torch.int8), ("logp", (T, n), torch.float32), ("rowlogp", (T, 2 * n), torch.float32),
        ("val_all", (T + 1, n), torch.float32), ("rew", (T, n), torch.float32), ("done", (T, n), torch.uint8),
        ("stats", (T, n, 2), torch.int32))}
    b["val"], b["last_val"] = b["val_all"][:T], b["val_all"][T]
    return b


def ensure_env(agent):
    """The agent's mazes and its [T, N] buffers, on first use."""
    if agent.venv is not None:
        return
    n, T, d = agent.n_envs, agent.horizon, agent.device
    base = int(agent.env_config.get("seed_base", 0)) if agent.env_config else random.getrandbits(32)
    kw = {k: v for k, v in agent._env_kwargs().items() if k != "seed_base"}
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(base) + np.uint64(agent.dp.rank * n)
    agent.venv = VecMaze(n, seeds=seeds, device=d, **kw)
    b = agent._bufs = step_buffers(T, n, d, zeroed=True)
    b["adv"] = torch.zeros((T, n), dtype=torch.float32, device=d)
    b["rtg"] = torch.zeros((T, n), dtype=torch.float32, device=d)
    agent.venv.reset(obs=b["obs"][0], masks=b["masks"][0])
    agent._fresh = True


def carry_over(agent):
    """The next batch starts from the last observation (episodes continue)."""
    b = agent._bufs
    b["obs"][0].copy_(b["obs"][agent.horizon])
    b["masks"][0].copy_(b["masks"][agent.horizon])


def env_step(agent, b, t, events=None):
    """The env half of step t: the actions of row t -> reward, done and episode stats of row t, the next state
    in row t + 1 (finished mazes reset).  events: the instrumented form, a (start, end) pair of HIP events stamped
    at the env-step kernel's own start / end."""
    nxt = dict(obs=b["obs"][t + 1], masks=b["masks"][t + 1])
    out = dict(reward=b["rew"][t], done=b["done"][t], ep_stats=b["stats"][t])
    if events is None:
        agent.venv.step(b["act"][t], auto_reset=True, **nxt, **out)
    else:
        agent.venv.step(b["act"][t], auto_reset=2, **nxt, **out, events=events)
        agent.venv.reset_done(**nxt)


def policy_step(agent, b, t, heads, offset, offset_dev=None, value=False, events=None):
    """Step t of a rollout into the buffers ``b``.  value: V(row t) from a critic launch of its own.  Actor trunk,
    heads and sampling (PPO.py:170-186): one launch after the front-end at small N (Actor.sample_actions), else
    the trunk's GEMMs + ops.head_act (Actor.act).  offset: the draw's Philox offset, a host integer, or relative
    to the device base ``offset_dev`` (the captured rollout's)."""
    n = agent.n_envs
    if value:
        agent.critic.value_into(b["obs"][t], b["val"][t])
    agent.actor.sample_actions(b["obs"][t].view(2 * n, 65), *heads, b["masks"][t].view(2 * n, 6), agent.sample_seed,
                               offset, actions=b["act"][t].view(2 * n, 2), logp=b["rowlogp"][t],
                               joint_logp=b["logp"][t], offset_dev=offset_dev)
    env_step(agent, b, t, events)


def _horizon_steps(agent, offset_dev=None):
    """``horizon`` policy steps, the values and the GAE into the agent's buffers: the launches of one
    fixed-horizon rollout, eager or under capture (offset_dev)."""
    b, n, T = agent._bufs, agent.n_envs, agent.horizon
    heads = agent.actor.heads()
    timed = agent.step_events
    for t in range(T):
        pair = None
        if timed is not None:
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for e in pair:
                e.record()  # materialise the events; the launch re-stamps them
            timed.append(pair)
        policy_step(agent, b, t, heads, t if offset_dev is not None else agent._sample_offset + t, offset_dev,
                    value=not BATCHED_CRITIC, events=pair)
    if offset_dev is None:
        agent._sample_offset += T
    if BATCHED_CRITIC:  # V(s_0 .. s_T-1) (and V(s_T) for the bootstrap) in one launch
        rows = T + 1 if agent.bootstrap else T
        agent.critic.value_into(b["obs"][:rows].reshape(rows * n, -1), b["val_all"][:rows].reshape(rows * n))
    elif agent.bootstrap:  # (the per-step values' arithmetic for V(s_T) too)
        agent.critic.value_into(b["obs"][T], b["last_val"])
    ops.gae(b["rew"], b["val"], b["done"], last_value=b["last_val"] if agent.bootstrap else None,
            gamma=agent.discount_rate, lam=agent.lam, adv=b["adv"], rtg=b["rtg"])
    return b


def fixed_horizon(agent):
    """Advance every maze ``horizon`` steps; fills the agent's [T, N] buffers and returns them.  The weights are
    fixed during the rollout: packed once, not per step.  The side-stream maze pre-generation is queued once, after
    the last step (VecMaze.defer_pregen): the steps' kernels get the GPU to themselves.  With ``agent.step_events``
    a list, every env step appends its (start, end) events to it."""
    venv = agent.venv
    with x3.cached_packs():
        venv.defer_pregen = True
        try:
            return _horizon_steps(agent)
        finally:
            venv.defer_pregen = False
            venv.flush_pregen()


class Replay:
    """The captured rollout's state: the HIP graph, what its launches hold by value (``key``: a change
    re-captures), whether the uncaptured first rollout has run, and the device base of the sampler's Philox offset
    with the host's idea of its value."""

    def __init__(self):
        self.graph = self.key = self.ctr = self.ctr_val = None
        self.warm = False


def captured(agent):
    """fixed_horizon as a replay of a captured HIP graph (same kernels, same draws: the sampler reads its Philox
    base offset from the device).  At a few thousand mazes the ~15 launches per step are host-bound; a replay is
    one launch."""
    r, b, T = agent._replay, agent._bufs, agent.horizon
    key = (id(agent.venv), agent.flat.data.data_ptr(), T, id(b["obs"]), agent.sample_seed,
           float(agent.discount_rate), float(agent.lam), bool(agent.bootstrap))
    if r.graph is None or r.key != key:
        if not r.warm:  # the first rollout runs uncaptured (one-time host work: kernel attributes)
            r.warm = True
            return fixed_horizon(agent)
        r.graph = torch.cuda.CUDAGraph()
        r.ctr = torch.tensor([agent._sample_offset], dtype=torch.int64, device=agent.device)
        r.ctr_val = agent._sample_offset
        torch.cuda.synchronize(agent.device)
        agent.venv.capturing = True
        try:
            with torch.cuda.graph(r.graph):
                with x3.cached_packs():
                    _horizon_steps(agent, offset_dev=r.ctr)
                r.ctr += T
        finally:
            agent.venv.capturing = False
        r.key = key
    if r.ctr_val != agent._sample_offset:  # an uncaptured rollout ran in between
        r.ctr.fill_(agent._sample_offset)
    r.graph.replay()
    agent._sample_offset += T
    r.ctr_val = agent._sample_offset
    agent.venv._kick_pregen()  # refill the next mazes the replay's resets consumed
    return b


def horizon_batch(agent):
    """The reference's 8-tuple (PPO.py:151-152) from one fixed-horizon rollout, samples flattened time-major."""
    b = agent.rollout()
    T, n = agent.horizon, agent.n_envs
    B = T * n
    st = b["stats"].reshape(B, 2)
    fin = st[:, 0] > 0
    out = (b["obs"][:T].reshape(B, 2, 65).clone(), b["act"].reshape(B, 2, 2).float(), b["logp"].reshape(B).clone(),
           st[fin, 1].tolist(), st[fin, 0].tolist(), b["masks"][:T].reshape(B, 2, 6).bool(),
           b["adv"].reshape(B).clone(), b["val"].reshape(B).clone())
    carry_over(agent)
    return out


@torch.no_grad()
def episode_batch(agent):
    """PPO.get_batch (PPO.py:89-152) over ``n_envs`` mazes, whole episodes only.

    Every maze is reset (PPO.py:104) and all step together.  The batch ends
    at the first step t* after which the steps of completed episodes (all
    mazes) exceed ``batch_size`` (per rank under DP) -- with one maze that is
    the reference's rule, the first episode end after more than
    ``batch_size`` steps (PPO.py:126-141).  Episodes still running at t* are
    dropped (the reference keeps only complete episodes).  Samples are
    ordered maze by maze, each maze's episodes in time order (one maze: the
    reference's order), and GAE runs on whole episodes (PPO.py:133; the
    episode-parallel walk of mm_gae_ex, bit-exact).  No step past t* may
    leave a trace (a maze finishing there would draw its next maze from its
    RNG stream, which the reference never does): after step t at most n (t + 1) steps
    can belong to completed episodes, so the steps before
    t_min = batch_size // n run in chunks of ``episode_chunk`` with one host
    synchronisation per chunk.  From t_min on the chunks grow geometrically
    (1, 2, 4, ... up to ``episode_chunk`` steps) from an environment
    snapshot: when the stop step falls inside a chunk, the environment is
    rewound to the chunk's start and only the steps up to t* are replayed
    with the recorded actions, so neither the MT19937 streams nor the
    sampler's Philox offset carry any trace of the overshoot into the next
    batch.  Every step takes the fixed-horizon rollout's value arithmetic
    (value_into: the fused fp32 kernel), so a network's stored values do not
    depend on the batch mode.
    """
    agent._arm_range_flag()
    ensure_env(agent)
    n, dev, venv = agent.n_envs, agent.device, agent.venv
    limit = agent.batch_size // agent.dp.world
    if agent._fresh:  # the state at the batch's first step
        obs0, masks0 = agent._bufs["obs"][0].clone(), agent._bufs["masks"][0].clone()
    else:
        obs0 = torch.empty((n, 2, 65), dtype=torch.float32, device=dev)
        masks0 = torch.empty((n, 2, 6), dtype=torch.uint8, device=dev)
        venv.reset(obs=obs0, masks=masks0)  # PPO.py:104
    agent._fresh = False
    heads = agent.actor.heads()
    chunks = []
    last_end = torch.full((n,), -1, dtype=torch.int64, device=dev)
    t0, t_stop, end_at_stop = 0, None, None
    t_min = limit // n  # the first step after which the batch can be full
    tail = 1  # the next chunk length past t_min
    agent._episode_replayed = 0
    with x3.cached_packs():  # the weights are fixed during the batch: packed once, not per step
        while t_stop is None:
            if t0 < t_min:
                C, snap = min(agent.episode_chunk, t_min - t0), None
            else:
                C, tail = tail, min(2 * tail, agent.episode_chunk)
                snap, off0 = venv.snapshot(), agent._sample_offset
            ch = step_buffers(C, n, dev, zeroed=False)
            ch["obs"][0].copy_(obs0)
            ch["masks"][0].copy_(masks0)
            for t in range(C):
                policy_step(agent, ch, t, heads, agent._sample_offset, value=True)
                agent._sample_offset += 1
            chunks.append(ch)
            obs0, masks0 = ch["obs"][C], ch["masks"][C]
            # completed-episode steps after each step of the chunk: sum over mazes of (last end + 1)
            tt = torch.arange(t0, t0 + C, device=dev).view(C, 1)
            ends = torch.where(ch["done"].bool(), tt, torch.full_like(tt, -1))
            ends = torch.maximum(torch.cummax(ends, 0).values, last_end.view(1, n))
            filled = (ends + 1).sum(1)
            hit = torch.nonzero(filled > limit)
            if hit.numel():  # one host synchronisation per chunk; only a tail chunk can hit
                k = int(hit[0, 0])
                t_stop, end_at_stop = t0 + k, ends[k]
                if k + 1 < C:  # overshoot: rewind to the chunk's start, replay steps t0 .. t* only
                    venv.restore(snap)
                    for t in range(k + 1):
                        env_step(agent, ch, t)
                    agent._sample_offset = off0 + k + 1
                    agent._episode_replayed = k + 1
            else:
                last_end = ends[-1]
                t0 += C
    Ts = t_stop + 1  # == the steps kept (the last chunk may hold discarded steps past t_stop)
    cat = {k: torch.cat([c[k][:c["act"].shape[0]] for c in chunks], 0)[:Ts]
           for k in ("obs", "masks", "act", "logp", "val", "rew", "done", "stats")}
    adv, rtg = ops.gae(cat["rew"], cat["val"], cat["done"], gamma=agent.discount_rate, lam=agent.lam)
    keep = torch.arange(Ts, device=dev).view(Ts, 1) <= end_at_stop.view(1, n)
    nt = torch.nonzero(keep.t())  # (maze, t), maze-major, t ascending
    flat = nt[:, 1] * n + nt[:, 0]
    B = flat.numel()
    pick = lambda x, *shape: x.reshape(Ts * n, *shape)[flat]  # noqa: E731
    st = pick(cat["stats"], 2)
    fin = st[:, 0] > 0
    out = (pick(cat["obs"], 2, 65), pick(cat["act"], 2, 2).float(), pick(cat["logp"]),
           st[fin, 1].tolist(), st[fin, 0].tolist(), pick(cat["masks"], 2, 6).bool(), pick(adv), pick(cat["val"]))
    agent._episode_info = dict(t_stop=t_stop, samples=B, rtg=pick(rtg), act=cat["act"], done=cat["done"])
    return out
