"""PPO over N parallel mazes on one or more MI355X -- the reference's PPO API.

Mirrors ``PPO`` of the reference (PPO.py:11-238): same constructor arguments,
same methods (train, get_batch, get_action, get_log_probs, get_state_values,
get_GAEs, get_rtgs, decay_lr, save/load_parameters), same checkpoint dict
(``actor``, ``critic``, ``actor_optim``, ``critic_optim``) so ``PPO.pth`` files
move both ways.  What changes is where the work runs:

* rollout: ``n_envs`` mazes step together in HBM (VecMaze, HIP kernels); per
  step one actor call on all [2N, 65] agent rows, one sampler kernel (masked
  Categorical + Bernoulli, PPO.py:170-186) and one env-step kernel, then one
  critic call on every step's [N, 130] observations.  No host synchronisation
  inside the rollout.  The buffers, the step and the collectors (fixed horizon, its
  captured replay, whole episodes) live in marlmaze.rollout; ``rollout``,
  ``get_batch``, ``_ensure_env`` and ``_carry_over`` here are calls of them.
* GAE: one HIP scan over the time-major [T, N] buffers (PPO.get_GAEs,
  PPO.py:193-203, bit-exact fp32).
* update: the clipped-surrogate + value-MSE minibatch loop of PPO.py:46-85,
  both losses in one backward, one flat gradient all-reduce under data
  parallelism (marlmaze.dist), clip_grad_norm_ per network, Adam.

Rollout semantics: the reference collects whole episodes from ONE maze until
more than ``batch_size`` steps are stored (PPO.py:108-141).  Here every maze
advances ``horizon`` steps per batch and episodes continue across batches; a
segment that ends mid-episode is bootstrapped with V(s_T) (``bootstrap=True``)
or treated as an episode end exactly like the reference's last step
(``bootstrap=False``).  The minibatch loop keeps the reference's quirk Q8
(it spans ``batch_size``, not the number of samples collected).
"""
import math
import os
import random
import warnings

import numpy as np
import torch

from . import _lib, networks, ops, rollout, update, x3
from .dist import DP
from .networks import Actor, Critic

MODEL_PATH = "PPO.pth"  # PPO.py:9 (CWD-relative)
# the update's critic (forward, value loss, backward) on a side stream beside the actor's kernels: the two
# networks share nothing until the loss values and the optimizer step.  At small minibatches (BASELINE
# configs[1]: 26,214 samples) the kernels of either network leave most CUs idle, and at the headline's 209,715
# the critic's kernels still fill the actor's tails: measured (same box, alternating) configs[1] 5.25M ->
# 5.38M env-steps/s, headline 6.96M -> 7.07M, f16 share 8.76M -> 8.95M.  MARLMAZE_CRITIC_STREAM=on (default)
# / off / auto (side stream up to CRITIC_STREAM_MAX_SAMPLES samples per minibatch)
CRITIC_STREAM = os.environ.get("MARLMAZE_CRITIC_STREAM", "on")
CRITIC_STREAM_MAX_SAMPLES = int(os.environ.get("MARLMAZE_CRITIC_STREAM_MAX", "65536"))


def _ppo_loss_fwd(heads, mk, a8, old_logp, adv, clip):
    """mm_ppo_loss: (coef [M] = d loss / d logp, per-workgroup partial sums of the surrogate)."""
    L = _lib.lib()
    M = old_logp.shape[0]
    old_logp, adv = old_logp.contiguous(), adv.contiguous()
    coef = torch.empty(M, dtype=torch.float32, device=heads.device)
    part = torch.empty(L.mm_ppo_loss_partials(M), dtype=torch.float32, device=heads.device)
    _lib.check(L.mm_ppo_loss(_lib.ptr(heads), _lib.ptr(mk), _lib.ptr(a8), _lib.ptr(old_logp), _lib.ptr(adv), M,
                             float(clip), _lib.ptr(coef), _lib.ptr(part), _lib.stream_ptr()), "mm_ppo_loss")
    return coef, part


def _ppo_loss_bwd(heads, mk, a8, coef, dloss):
    """mm_ppo_loss_bwd: d loss / d heads [2M, 6] (dloss: a 1-element device tensor)."""
    dz = torch.empty_like(heads)
    _lib.check(_lib.lib().mm_ppo_loss_bwd(_lib.ptr(heads), _lib.ptr(mk), _lib.ptr(a8), _lib.ptr(coef),
                                          _lib.ptr(dloss), coef.shape[0], _lib.ptr(dz), _lib.stream_ptr()),
               "mm_ppo_loss_bwd")
    return dz


def _ppo_loss_ent_fwd(heads, mk, a8, old_logp, adv, clip, ent_coef):
    """mm_ppo_loss_ent: (coef, partial) as _ppo_loss_fwd, and the diagnostics' per-workgroup partials
    [partials, PPO_STAT_WORDS] for update.ppo_stats_final."""
    L = _lib.lib()
    M = old_logp.shape[0]
    old_logp, adv = old_logp.contiguous(), adv.contiguous()
    coef = torch.empty(M, dtype=torch.float32, device=heads.device)
    n = L.mm_ppo_loss_partials(M)
    part = torch.empty(n, dtype=torch.float32, device=heads.device)
    stat_part = torch.empty((n, _lib.PPO_STAT_WORDS), dtype=torch.float32, device=heads.device)
    _lib.check(L.mm_ppo_loss_ent(_lib.ptr(heads), _lib.ptr(mk), _lib.ptr(a8), _lib.ptr(old_logp), _lib.ptr(adv), M,
                                 float(clip), float(ent_coef), _lib.ptr(coef), _lib.ptr(part), _lib.ptr(stat_part),
                                 _lib.stream_ptr()), "mm_ppo_loss_ent")
    return coef, part, stat_part


def _ppo_loss_ent_bwd(heads, mk, a8, coef, dloss, ent_coef):
    """mm_ppo_loss_ent_bwd: d (surrogate - ent_coef mean H) / d heads [2M, 6]."""
    dz = torch.empty_like(heads)
    _lib.check(_lib.lib().mm_ppo_loss_ent_bwd(_lib.ptr(heads), _lib.ptr(mk), _lib.ptr(a8), _lib.ptr(coef),
                                              _lib.ptr(dloss), coef.shape[0], float(ent_coef), _lib.ptr(dz),
                                              _lib.stream_ptr()), "mm_ppo_loss_ent_bwd")
    return dz


def _u8(masks):
    masks = masks.contiguous()
    return masks.view(torch.uint8) if masks.dtype == torch.bool else masks.to(torch.uint8)


class _PolicyLoss(torch.autograd.Function):
    """-mean(min(r A, clamp(r, 1-clip, 1+clip) A)), r = exp(logp - old_logp),
    logp = sum over the two agents of get_log_probs (PPO.py:62-72, 154-168),
    straight from the [2M, 6] head logits (mm_ppo_loss, mm_ppo_loss_bwd), with
    autograd (the update itself runs the kernels without it)."""

    @staticmethod
    def forward(ctx, heads, masks, act, old_logp, adv, clip):
        heads = heads.contiguous()
        mk = _u8(masks)
        a8 = act.to(torch.int8).contiguous()
        coef, part = _ppo_loss_fwd(heads, mk, a8, old_logp, adv, clip)
        ctx.save_for_backward(heads, mk, a8, coef)
        return -part.sum() / old_logp.shape[0]

    @staticmethod
    def backward(ctx, dloss):
        heads, mk, a8, coef = ctx.saved_tensors
        dz = _ppo_loss_bwd(heads, mk, a8, coef, dloss.reshape(1).to(torch.float32).contiguous())
        return dz, None, None, None, None, None


class PPO:
    def __init__(self, agent_amount, epochs=500, batch_size=15000, lr=0.0002, discount_rate=0.99, lam=0.95,
                 updates_per_batch=5, clip=0.2, max_grad=0.5, *, n_envs=4096, horizon=None, env_config=None,
                 seed=3234, sample_seed=None, device=None, model_path=MODEL_PATH, load=True, parity_mode=True,
                 bootstrap=True, dp=None, verbose=True, save=True, episode_batches=False,
                 episode_chunk=64, dtype="f32", graph_rollout=False, ent_coef=0.0, diagnostics=False):
        self.maze = None  # wired by Maze.__init__ (maze.py:39-42), as in the reference
        self.dp = dp if dp is not None else DP.single()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        # networks are built on the CPU right after the seed, like PPO.py:7,16-17; only the CPU
        # generator is seeded (torch.manual_seed would also reset the caller's CUDA streams) and
        # its state is restored afterwards
        g = torch.random.get_rng_state()
        torch.default_generator.manual_seed(seed)
        # dtype "f32": the networks' GEMMs at fp32-class accuracy (x2 by default: two fp16 planes per operand,
        # three f16 MFMAs per product, range-guarded; x3 = bf16x3 on request); "f16": fp16 MFMA operands with
        # fp32 accumulation, storage and Adam (BASELINE configs[4]); the parameters are fp32 either way
        if dtype not in ("f32", "f16"):
            raise ValueError(f"dtype must be 'f32' or 'f16', not {dtype!r}")
        self.dtype = dtype
        # the fp32-class GEMM arithmetic: networks.FP32_GEMM, "x2" (two fp16 planes, three MFMAs per product)
        # unless MARLMAZE_FP32_GEMM=x3 (three bf16 planes, six)
        prec = networks.FP32_GEMM if dtype == "f32" else "f16"
        self.gemm_prec = prec
        self.actor = Actor([264, 264, 264], parity_mode=parity_mode, gemm_prec=prec).to(self.device)
        self.critic = Critic(agent_amount, hidden_sizes=[64, 64], gemm_prec=prec).to(self.device)
        torch.random.set_rng_state(g)
        # Adam (PPO.py:18-19)
        self.flat = None
        if self.device.type == "cuda":
            # both networks in one flat parameter buffer (marlmaze.update): the explicit backward writes
            # into its gradient twin, one all-reduce under DP, clip + Adam for both in two launches
            a = self.actor
            order = [p for n, p in a.named_parameters() if not n.startswith(("move_head", "mark_head"))]
            order += [a.move_head.weight, a.mark_head.weight, a.move_head.bias, a.mark_head.bias]
            self.flat = update.FlatParams([order, list(self.critic.parameters())],
                                          adjacent=[(a.move_head.weight, a.mark_head.weight),
                                                    (a.move_head.bias, a.mark_head.bias)])
            self.dp.broadcast_tensor(self.flat.data)
            mom = (torch.zeros_like(self.flat.data), torch.zeros_like(self.flat.data))
            self.actor_optim = update.FlatAdam(self.flat, 0, self.actor.parameters(), lr=lr, moments=mom)
            self.critic_optim = update.FlatAdam(self.flat, 1, self.critic.parameters(), lr=lr, moments=mom)
        else:  # the host (CPU torch) form, for CPU runs and tests
            self.dp.broadcast_params([self.actor, self.critic])
            self.actor_optim = torch.optim.Adam(self.actor.parameters(), lr=lr)
            self.critic_optim = torch.optim.Adam(self.critic.parameters(), lr=lr)
        self._one = torch.ones(1, dtype=torch.float32, device=self.device)  # d loss / d loss

        self.agent_amount = agent_amount
        self.epochs = epochs
        self.batch_size = batch_size
        self.lr = lr
        self.discount_rate = discount_rate
        self.lam = lam
        self.updates_per_batch = updates_per_batch
        self.mbatch_size = self.batch_size // 5
        self.clip = clip
        self.max_grad = max_grad
        # entropy bonus (no reference counterpart): the update minimises surrogate - ent_coef * mean joint entropy
        # of the masked move distributions and the mark Bernoullis.  With a bonus, or with ``diagnostics``, every
        # minibatch also yields [entropy, approx_kl, clip_frac, ratio_max] (``last_update_stats`` [K, 4]); with
        # neither (the default) the update is the reference's, launch for launch.  Not part of the checkpoint
        self.ent_coef = float(ent_coef)
        if not math.isfinite(self.ent_coef):
            raise ValueError(f"ent_coef must be finite, not {ent_coef!r}")
        self.diagnostics = bool(diagnostics)
        self.last_update_stats = None

        self.n_envs = int(n_envs)
        self.horizon = int(horizon) if horizon else max(1, math.ceil(batch_size / (self.n_envs * self.dp.world)))
        self.env_config = env_config
        self.bootstrap = bootstrap
        self.episode_batches = bool(episode_batches)  # the reference's whole-episode batches (rollout.episode_batch)
        self.episode_chunk = int(episode_chunk)
        self._fresh = False  # the env was just reset (its first batch needs no reset of its own)
        self.sample_seed = (sample_seed if sample_seed is not None else random.getrandbits(63)) + 7919 * self.dp.rank
        self._sample_offset = 0
        self._shuffle_gen = None
        self.model_path = model_path
        self.verbose = verbose and self.dp.rank == 0
        self.save = save
        self.venv = None
        self._bufs = None
        self.history = []
        self.step_events = None  # list -> rollout records (start, end) events around each env step
        # capture the fixed-horizon rollout (every step's actor trunk, head + sampler and env step, the critic
        # and the GAE) in one HIP graph and replay it (rollout.captured)
        self.graph_rollout = bool(graph_rollout)
        self._replay = rollout.Replay()
        self.range_redos = 0  # updates redone at x3 by the range guard (_range_guarded)
        self.range_switched = False  # the rollout's operands left the fp16 range: the networks now run x3
        self.batches_discarded = 0  # batches the range guard threw away (their rollout left the fp16 range)
        self.last_update_discarded = False
        self._flag_armed = False  # a rollout cleared the range flag at its start: the next update reads its flag
        if load:
            self.load_parameters()

    # ------------------------------------------------------------------
    # environment + buffers
    # ------------------------------------------------------------------
    def _env_kwargs(self):
        if self.env_config is not None:
            return dict(self.env_config)
        m = self.maze
        if m is None:
            return dict(default_size=(10, 10), max_timestep=1200)
        return dict(default_size=tuple(m.default_size), max_timestep=m.max_timestep, difficulty=m.difficulty,
                    rand_start=m.rand_start, rand_sizes=m.rand_sizes, rand_range=tuple(m.rand_range))

    def _ensure_env(self):
        rollout.ensure_env(self)

    # ------------------------------------------------------------------
    # rollout (PPO.get_batch, PPO.py:89-152): marlmaze.rollout
    # ------------------------------------------------------------------
    def _arm_range_flag(self):
        """A rollout starts: clear the library's range flag, so that what the next update reads as the
        rollout's flag (``pre``, _range_guarded) covers this batch's GEMMs and nothing older."""
        if self.flat is not None and self.gemm_prec != "x3":
            x3.range_flag(clear=True)
            self._flag_armed = True

    @torch.no_grad()
    def rollout(self):
        """Advance every maze ``horizon`` steps; fills and returns the [T, N] buffers (``_bufs``).  With
        ``graph_rollout`` (and no ``step_events`` instrumentation): a replay of the captured rollout."""
        self._arm_range_flag()
        self._ensure_env()
        if self.graph_rollout and self.step_events is None:
            return rollout.captured(self)
        return rollout.fixed_horizon(self)

    @property
    def _graph(self):
        return self._replay.graph

    def _carry_over(self):
        rollout.carry_over(self)

    def get_batch(self):
        """Reference 8-tuple (PPO.py:151-152).  Default: every maze advances
        ``horizon`` steps, samples flattened time-major.  ``episode_batches``:
        whole episodes only (rollout.episode_batch)."""
        return rollout.episode_batch(self) if self.episode_batches else rollout.horizon_batch(self)

    # ------------------------------------------------------------------
    # update (PPO.py:46-85)
    # ------------------------------------------------------------------
    def policy_logp(self, obs, act, masks):
        """Sum over agents of get_log_probs (PPO.py:66-68), one actor call on [2M, 65]."""
        M = obs.shape[0]
        ml, kl = self.actor(obs.reshape(2 * M, 65))
        mk = masks.reshape(2 * M, 6).bool()
        a = act.reshape(2 * M, 2)
        ml = ml.masked_fill(~mk[:, 0:5], float("-inf"))
        lp = torch.log_softmax(ml, dim=-1).gather(1, a[:, 0:1].long()).squeeze(1)
        kl = kl.squeeze(1).masked_fill(~mk[:, 5], float("-inf"))
        p = torch.sigmoid(kl)
        p = torch.where(a[:, 1] != 0, p, 1 - p)
        lp = (lp + torch.log(p)).view(M, 2)
        return lp[:, 0] + lp[:, 1]

    @property
    def stats_on(self):
        """The update runs the entropy form of the policy loss and fills ``last_update_stats``."""
        return self.diagnostics or self.ent_coef != 0.0

    def minibatch_grads(self, obs, act, old_logp, adv, rtg, masks, out=None, stats_out=None):
        """Losses of PPO.py:62-80 and their gradients in every parameter's .grad
        (before the all-reduce, the clipping and Adam).  Returns (actor_loss,
        critic_loss) as 0-dim tensors (views of ``out`` [2] when given).
        The actor loss is the clipped surrogate, also with an entropy bonus (whose
        gradient is in .grad): comparable with the reference's.  With ``stats_on``,
        ``stats_out`` [4] (optional) receives [entropy, approx_kl, clip_frac,
        ratio_max] of this minibatch.

        On the GPU: no autograd.  The critic and actor forwards keep what their
        backwards need; the policy loss (mm_ppo_loss) and the value loss
        (mm_mse_loss) hand d loss / d logits and d loss / dV straight to the
        explicit backwards (Actor / Critic .train_backward), which write into the
        flat gradient buffer."""
        if not obs.is_cuda:
            return self._minibatch_grads_host(obs, act, old_logp, adv, rtg, masks, stats_out)
        M = obs.shape[0]
        a8 = (act if act.dtype == torch.int8 else act.to(torch.int8)).contiguous()
        mk = _u8(masks)
        if out is None:
            out = torch.empty(2, dtype=torch.float32, device=obs.device)
        # the critic beside the actor (CRITIC_STREAM): its launches go to the device's "critic" side stream, which
        # waits for the weight packs; this stream waits for it before the loss values and the optimizer.  Off:
        # the same launches on this stream, in the order written (the same results bit for bit)
        beside = CRITIC_STREAM == "on" or (CRITIC_STREAM == "auto" and M <= CRITIC_STREAM_MAX_SAMPLES)
        with x3.cached_packs():
            # every weight pack of both networks' forward and backward in one launch per precision, and each
            # backward's bias-gradient and weight-gradient reductions together at its end
            x3.pack_many(self.critic.pack_specs() + self.actor.pack_specs())
            with _lib.on_side(_lib.side_stream("critic", obs.device) if beside else None) as critic_side:
                xc = obs.reshape(M, -1)
                if self.critic.fused_update_ok(xc):  # (x2, the reference widths, M >= the B-resident threshold)
                    _, mse_part = self.critic.train_update_fused(xc, rtg)
                else:
                    V, csaved = self.critic.train_forward(xc)
                    mse_part, dv = update.mse_loss(V, rtg)
                    with x3.deferred():
                        self.critic.train_backward(csaved, dv)
            heads, asaved = self.actor.train_forward(obs.reshape(2 * M, 65))
            kappa = None
            if self.stats_on:  # the same loss with the entropy bonus in dz, and the diagnostics' partial sums
                coef, ppo_part, stat_part = _ppo_loss_ent_fwd(heads, mk, a8, old_logp, adv, self.clip, self.ent_coef)
                dz = _ppo_loss_ent_bwd(heads, mk, a8, coef, self._one, self.ent_coef)
                if self.ent_coef != 0.0 and self.gemm_prec != "x3":
                    # the fp16-plane backward GEMMs expect max |dz| of a few / M (a mean of O(1) terms); where the
                    # bonus carries the gradient it is ent_coef times that, into fp16's subnormals.  dz times a
                    # power of two, the actor's gradients divided by it again: exact, on the device
                    kappa = update.pow2_norm(dz, M / 4.0)  # kappa max|dz| in [4 / M, 8 / M)
                    update.scale_by(dz, kappa[0:1])
            else:
                coef, ppo_part = _ppo_loss_fwd(heads, mk, a8, old_logp, adv, self.clip)
                dz = _ppo_loss_bwd(heads, mk, a8, coef, self._one)
            with x3.deferred():
                self.actor.train_backward(asaved, dz)
            if kappa is not None:
                update.scale_by(self.flat.seg_view(self.flat.grad, 0), kappa[1:2])
            critic_side.join(mse_part)
            update.losses_final(ppo_part, mse_part, M, out)
            if self.stats_on and stats_out is not None:
                update.ppo_stats_final(stat_part, M, stats_out)
        return out[0], out[1]

    def policy_entropy(self, obs, masks):
        """The joint entropy [M] of the policy at ``obs``: per agent the masked move Categorical's plus, where the
        mark is allowed, the mark Bernoulli's (torch.distributions; a row with no legal move counts 0)."""
        M = obs.shape[0]
        ml, kl = self.actor(obs.reshape(2 * M, 65))
        mk = masks.reshape(2 * M, 6).bool()
        legal = mk[:, 0:5].any(1)
        mv = mk[:, 0:5] | ~legal[:, None]  # (a row with no legal move: any finite distribution, then times 0)
        h_move = torch.distributions.Categorical(logits=ml.masked_fill(~mv, float("-inf"))).entropy() * legal
        kl = torch.where(mk[:, 5], kl.squeeze(1), torch.zeros_like(kl.squeeze(1)))
        h_mark = torch.distributions.Bernoulli(logits=kl).entropy() * mk[:, 5]
        return (h_move + h_mark).view(M, 2).sum(1)

    def _minibatch_grads_host(self, obs, act, old_logp, adv, rtg, masks, stats_out=None):
        """The CPU torch form (autograd, the reference's formulas; the entropy bonus and the diagnostics with
        torch.distributions)."""
        V = self.critic(obs).view(-1)
        cur = self.policy_logp(obs, act, masks)
        d = cur - old_logp
        ratio = torch.exp(d)
        s1 = ratio * adv
        s2 = torch.clamp(ratio, 1 - self.clip, 1 + self.clip) * adv
        actor_loss = -torch.mean(torch.min(s1, s2))
        critic_loss = torch.nn.functional.mse_loss(V, rtg)
        total = actor_loss + critic_loss
        if self.stats_on:
            entropy = self.policy_entropy(obs, masks).mean()
            if self.ent_coef != 0.0:
                total = total - self.ent_coef * entropy
            if stats_out is not None:
                with torch.no_grad():
                    outside = (ratio < 1 - self.clip) | (ratio > 1 + self.clip)
                    stats_out.copy_(torch.stack([entropy.detach(), (torch.expm1(d) - d).mean(),
                                                 outside.to(ratio.dtype).mean(), ratio.max()]))
        self.actor_optim.zero_grad(set_to_none=True)
        self.critic_optim.zero_grad(set_to_none=True)
        total.backward()  # disjoint parameters: same grads as two backwards
        return actor_loss.detach(), critic_loss.detach()

    def minibatch_step(self, obs, act, old_logp, adv, rtg, masks, out=None, stats_out=None):
        """One iteration of PPO.py:58-85: losses, gradients, all-reduce (DP),
        clip_grad_norm_ per network, Adam.  Returns (aloss, closs, gnorm_a,
        gnorm_c) as 0-dim tensors (views of ``out`` [4] when given).
        ``stats_out``: as minibatch_grads.

        On the GPU the step is the minibatch_grads launches, one all-reduce of the
        flat gradient buffer under DP (sums; the 1 / world scale is folded into
        the optimizer kernel), and mm_clip_adam for both networks."""
        if self.flat is None:
            return self._minibatch_step_host(obs, act, old_logp, adv, rtg, masks, stats_out)
        if out is None:
            out = torch.empty(4, dtype=torch.float32, device=obs.device)
        self.minibatch_grads(obs, act, old_logp, adv, rtg, masks, out=out[0:2], stats_out=stats_out)
        scale = 1.0
        if self.dp.active:
            self.dp.allreduce_sum(self.flat.grad)
            scale = 1.0 / self.dp.world
        update.clip_adam([self.actor_optim, self.critic_optim], self.max_grad, norms=out[2:4], grad_scale=scale)
        return out[0], out[1], out[2], out[3]

    def _minibatch_step_host(self, obs, act, old_logp, adv, rtg, masks, stats_out=None):
        actor_loss, critic_loss = self._minibatch_grads_host(obs, act, old_logp, adv, rtg, masks, stats_out)
        params = list(self.actor.parameters()) + list(self.critic.parameters())
        self.dp.allreduce_grads(params)
        gna = torch.nn.utils.clip_grad_norm_(self.actor.parameters(), self.max_grad)
        gnc = torch.nn.utils.clip_grad_norm_(self.critic.parameters(), self.max_grad)
        self.actor_optim.step()
        self.critic_optim.step()
        return actor_loss, critic_loss, gna.detach(), gnc.detach()

    def update(self, b_obs, b_act, b_logp, b_masks, b_advs, b_vals, index_list=None, generator=None):
        """Update body of PPO.train; returns per-minibatch (aloss, closs, gnorm_a, gnorm_c) [K, 4]."""
        b_rtgs = b_advs + b_vals
        mean, std = self.dp.global_mean_std(b_advs)
        b_advs = (b_advs - mean) / (std + 1e-10)
        B = b_obs.shape[0]
        if index_list is None:
            if generator is None:  # a per-rank stream (sample_seed differs by rank), not the global RNG
                if self._shuffle_gen is None or self._shuffle_gen.device != b_obs.device:
                    self._shuffle_gen = torch.Generator(device=b_obs.device)
                    self._shuffle_gen.manual_seed(self.sample_seed ^ 0x5EED)
                generator = self._shuffle_gen
            index_list = torch.randperm(B, device=b_obs.device, generator=generator)
        else:
            index_list = torch.as_tensor(index_list, device=b_obs.device, dtype=torch.long)
        # the reference's minibatch loop spans batch_size (Q8).  Under DP, or for a batch smaller than
        # batch_size (explicit horizon * n_envs < batch_size), the batch is used whole: exactly 5
        # minibatches of local_bs // 5 (a remainder of < 5 samples is left out, as the reference's
        # loop leaves out everything past batch_size)
        local_bs = min(self.batch_size // self.dp.world, B)
        whole = self.dp.active or local_bs < self.batch_size
        mb = local_bs // 5 if whole else self.mbatch_size
        if mb < 1:
            raise ValueError(f"batch of {B} samples per rank is too small for 5 minibatches")
        starts = list(range(0, 5 * mb, mb)) if whole else list(range(0, local_bs, mb))
        # the reference shuffles once per batch (PPO.py:48-49): gather the batch into that order once,
        # so every minibatch is a contiguous slice (same rows, no per-minibatch gathers)
        used = min(B, starts[-1] + mb)
        order = index_list[:used]
        p_obs, p_act, p_logp, p_advs, p_rtgs, p_masks = (t[order] for t in (b_obs, b_act, b_logp, b_advs, b_rtgs,
                                                                          b_masks))
        if p_obs.is_cuda:  # the fused policy-loss kernels take int8 actions and u8 masks: convert once
            p_act = p_act.to(torch.int8)
            p_masks = _u8(p_masks)
        K = self.updates_per_batch * len(starts)
        mbs = [(p_obs[s:s + mb], p_act[s:s + mb], p_logp[s:s + mb], p_advs[s:s + mb], p_rtgs[s:s + mb],
                p_masks[s:s + mb]) for s in starts]

        def passes():
            hist = torch.empty((K, 4), dtype=torch.float32, device=b_obs.device)
            stats = None
            if self.stats_on:  # [entropy, approx_kl, clip_frac, ratio_max] per minibatch (a redo's replace the first's)
                stats = self.last_update_stats = torch.empty((K, _lib.PPO_STAT_WORDS), dtype=torch.float32,
                                                             device=b_obs.device)
            k = 0
            for _ in range(self.updates_per_batch):
                self.decay_lr()
                for args in mbs:
                    kw = {"out": hist[k]} if self.flat is not None else {}
                    if stats is not None:
                        kw["stats_out"] = stats[k]
                    row = self.minibatch_step(*args, **kw)
                    if self.flat is None:
                        hist[k] = torch.stack(row)
                    k += 1
            if self.dp.active:  # local losses -> global-minibatch losses (equal shards); norms are already global
                self.dp.allreduce_sum(hist)
                hist /= self.dp.world
                if stats is not None:
                    self.dp.allreduce_update_stats(stats)
            return hist

        self.last_update_discarded = False
        if self.flat is None or self.gemm_prec == "x3":
            return passes()
        return self._range_guarded(passes)

    # ---- range guard of the fp16-plane GEMMs (x2, f16) ----
    def set_gemm_prec(self, prec):
        """The precision of both networks' GEMMs on the GPU ("x2", "x3" or "f16")."""
        assert prec in networks.GEMM_PRECISIONS
        self.gemm_prec = self.actor.gemm_prec = self.critic.gemm_prec = prec
        # a captured rollout holds the old precision's kernels: start over (the new precision's kernels run
        # uncaptured once, then they are captured)
        self._replay = rollout.Replay()

    def _range_guarded(self, passes):
        """Run the update passes; if any GEMM operand they converted to fp16 planes had |x s| >= 2^15 (the
        library's range flag, mm_gemm_range_flag) on any rank, restore the parameters and optimizer state and
        run the same passes again with the bf16x3 GEMMs (fp32's range).  A flag raised since the batch's rollout
        began (its actor GEMMs, on any rank) means this batch's actions and old log-probs did not come from the
        fp32 policy (an inf / NaN accumulator can become 0 through a ReLU): the update on it is thrown away
        (parameters and optimizer state restored, hist NaN, ``last_update_discarded``), and both networks run
        their GEMMs at x3 from now on (``train`` then collects a new batch).  One host synchronisation per
        update (the flags' read, DP.raised_on_any_rank: under DP every rank takes the same branch)."""
        # the flag raised since this agent's last rollout began (its actor GEMMs); a batch that did not come
        # from a rollout of this agent (update() on given tensors) has no rollout flag: a stale one is dropped
        pre = x3.range_flag(clear=True)
        if not self._flag_armed:
            pre.zero_()
        self._flag_armed = False
        snap = update.Snapshot(self.flat, (self.actor_optim, self.critic_optim))
        hist = passes()
        post = x3.range_flag(clear=True)
        pre_set, post_set = self.dp.raised_on_any_rank(pre, post)
        self.last_update_discarded = bool(pre_set)
        if pre_set:
            snap.restore()
            warnings.warn(f"marlmaze: a {self.gemm_prec} GEMM operand of the rollout reached |x| >= 2^15 (fp16 "
                          "planes): the update on this batch is discarded, and both networks run their GEMMs at "
                          "x3 (bf16x3, fp32 range) from now on")
            self.set_gemm_prec("x3")
            self.range_switched = True
            self.batches_discarded += 1
            hist.fill_(float("nan"))
            if self.last_update_stats is not None:
                self.last_update_stats.fill_(float("nan"))
            return hist
        if post_set:
            snap.restore()
            prec = self.gemm_prec
            self.set_gemm_prec("x3")
            try:
                hist = passes()
            finally:
                self.set_gemm_prec(prec)
            self.range_redos += 1
        return hist

    # ------------------------------------------------------------------
    # evaluation
    # ------------------------------------------------------------------
    def evaluate(self, episodes_per_env=1, greedy=True, n_envs=None, env_config=None, seed_base=0, eval_seed=0,
                 poll=16, record=False, par=False, episode_log=False):
        """How good is the policy: ``episodes_per_env`` whole episodes on each of ``n_envs`` fresh mazes, greedy or
        sampled, counted on the device; optionally rated against par and logged per episode.  Returns the result
        dict (with ``record``: and the recorded steps).  Training does not notice the call.  The arguments, the
        result and the driver itself: marlmaze.evaluate.evaluate_policy."""
        from .evaluate import evaluate_policy

        return evaluate_policy(self, episodes_per_env, greedy, n_envs, env_config, seed_base, eval_seed, poll, record,
                               par, episode_log)

    def train(self, eval_every=0, eval_kwargs=None):
        """PPO.train (PPO.py:22-44).  ``eval_every`` > 0: after every ``eval_every``-th epoch, evaluate(**eval_kwargs)
        is stored in that epoch's history entry under "eval" (and printed as one line)."""
        for epoch in range(self.epochs):
            b_obs, b_act, b_lp, b_sp, ep_lens, b_masks, b_advs, b_vals = self.get_batch()
            hist = self.update(b_obs, b_act, b_lp, b_masks, b_advs, b_vals)
            if self.last_update_discarded:  # the range guard threw the batch away (now at x3): collect another
                b_obs, b_act, b_lp, b_sp, ep_lens, b_masks, b_advs, b_vals = self.get_batch()
                hist = self.update(b_obs, b_act, b_lp, b_masks, b_advs, b_vals)
            episodes, mean_len, mean_short = self.dp.episode_stats(ep_lens, b_sp)  # all ranks' episodes
            stats = dict(epoch=epoch, episodes=episodes, mean_len=mean_len, mean_shortest=mean_short,
                         actor_loss=float(hist[-1, 0]), critic_loss=float(hist[-1, 1]))
            if self.stats_on:  # the last minibatch's, as the losses
                stats.update(zip(_lib.PPO_STAT_FIELDS, self.last_update_stats[-1].tolist()))
            self.history.append(stats)
            if self.verbose:  # PPO.py:37-44, condensed
                print(f"-------------------- Epoch #{epoch} --------------------")
                print(f"Mazes solved in current epoch: {stats['episodes']}")
                print(f"Average Exit Time: {stats['mean_len']}")
                print(f"Average Length of Shortest Path: {stats['mean_shortest']}", flush=True)
                if self.stats_on:
                    print(f"Policy entropy: {stats['entropy']:.4f}  approx KL: {stats['approx_kl']:.3g}  clipped: "
                          f"{stats['clip_frac']:.3f}  max ratio: {stats['ratio_max']:.3f}", flush=True)
            if eval_every > 0 and (epoch + 1) % eval_every == 0:
                from .evaluate import format_result

                stats["eval"] = self.evaluate(**(eval_kwargs or {}))
                if self.verbose:
                    print(format_result(stats["eval"]), flush=True)
            if self.save and self.dp.rank == 0:
                self.save_parameters()

    # ------------------------------------------------------------------
    # single-sample API of the reference
    # ------------------------------------------------------------------
    @torch.no_grad()
    def get_action(self, obs, action_mask, greedy=False):
        """PPO.get_action (PPO.py:170-186): ([move, mark], log_prob (1,1)).  ``greedy``: the most likely action
        (ops.act: the lowest-index legal move with the maximal logit, a mark where its logit is > 0) and its
        log-prob; no draw, the sampler's offset stays where it is."""
        ml, kl = self.actor(obs)
        mk = torch.as_tensor(np.asarray(action_mask, dtype=np.uint8), device=self.device).view(1, 6)
        if greedy:
            a, lp, _ = ops.act(ml, kl.reshape(-1), mk, mode="greedy")
        else:
            a, lp, _ = ops.sample(ml, kl.reshape(-1), mk, self.sample_seed, self._sample_offset)
            self._sample_offset += 1
        a = a.cpu().tolist()[0]
        return [a[0], a[1]], lp.view(1, 1)

    def get_log_probs(self, i, batch_obs, batch_actions, batch_masks):
        """PPO.get_log_probs (PPO.py:154-168)."""
        moves, marks = batch_actions[:, i, 0], batch_actions[:, i, 1]
        ml, kl = self.actor(batch_obs[:, i, :])
        ml = ml.masked_fill(~batch_masks[:, i, 0:5], float("-inf"))
        lp = torch.log_softmax(ml, dim=-1).gather(1, moves.long().view(-1, 1)).squeeze(1)
        kl = kl.squeeze(1).masked_fill(~batch_masks[:, i, 5], float("-inf"))
        p = torch.sigmoid(kl)
        p = torch.where(marks.to(torch.bool), p, 1 - p)
        return lp + torch.log(p)

    def get_state_values(self, batch_obs):
        return self.critic(batch_obs).squeeze()

    def get_GAEs(self, ep_rew, ep_values, ep_dones):
        """PPO.get_GAEs (PPO.py:193-203) on the GPU scan; returns a float64 array like the reference."""
        L = len(ep_rew)
        r = torch.as_tensor(np.asarray(ep_rew, np.float32), device=self.device).view(L, 1)
        v = torch.as_tensor(np.asarray([float(x) for x in ep_values], np.float32), device=self.device).view(L, 1)
        d = torch.as_tensor(np.asarray(ep_dones, np.uint8), device=self.device).view(L, 1)
        d[-1] = 1  # the reference's t+1 == L branch ends the episode
        adv, _ = ops.gae(r, v, d, gamma=self.discount_rate, lam=self.lam)
        return adv.view(L).cpu().numpy().astype(np.float64)

    def get_rtgs(self, batch_rew):
        """PPO.get_rtgs (PPO.py:205-214): logging helper, 0.995 discount."""
        rtgs = []
        for episode_rew in reversed(batch_rew):
            acc = 0
            for rew in reversed(episode_rew):
                acc = rew + 0.995 * acc
                rtgs.append(acc)
        rtgs.reverse()
        return rtgs

    def decay_lr(self):
        for opt in (self.actor_optim, self.critic_optim):  # PPO.py:216-220
            for group in opt.param_groups:
                group["lr"] *= 0.997

    def save_parameters(self):
        """PPO.py:222-230: the same four entries; tensors are saved on the CPU so
        the reference (CPU torch) can load the file as it loads its own."""
        def cpu(o):
            if torch.is_tensor(o):
                return o.detach().cpu()
            if isinstance(o, dict):
                return {k: cpu(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return type(o)(cpu(v) for v in o)
            return o

        torch.save(cpu({"actor": self.actor.state_dict(), "critic": self.critic.state_dict(),
                        "actor_optim": self.actor_optim.state_dict(),
                        "critic_optim": self.critic_optim.state_dict()}), self.model_path)

    def load_optim_state(self, opt, state):
        """Adam.load_state_dict, keeping this build's Adam: a state dict written
        by the reference (CPU torch.optim.Adam) loads into the flat GPU optimizer
        (marlmaze.update.FlatAdam) and back."""
        opt.load_state_dict(state)
        if self.flat is not None:
            x3.invalidate_packs()

    def load_parameters(self):
        if os.path.exists(self.model_path):
            sd = torch.load(self.model_path, weights_only=True, map_location=self.device)
            self.actor.load_state_dict(sd["actor"])
            self.critic.load_state_dict(sd["critic"])
            self.load_optim_state(self.actor_optim, sd["actor_optim"])
            self.load_optim_state(self.critic_optim, sd["critic_optim"])
            if self.verbose:
                print("successfuly loaded existing parameters")
            return True
        return False

