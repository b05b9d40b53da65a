"""The entropy bonus and the update's diagnostics in the host (CPU torch) form of the PPO update, and their
reduction across data-parallel ranks (gloo).  The GPU kernels' side: tests/test_gpu_entropy_loss.py.

The closed forms (per agent row, z the six head logits, mk the mask):
  H_move = -sum over legal j of p_j log p_j, p the softmax over the legal moves (0 for an underflowed p_j);
  H_mark = log1p(t) + a t / (1 + t), a = |z_5|, t = exp(-a), where the mark is allowed, else 0;
  H_i = the sum over the sample's two rows; d_i = logp_i - old_logp_i, r_i = exp(d_i);
  stats = [mean H_i, mean (expm1(d_i) - d_i), fraction of r_i outside [1 - clip, 1 + clip], max r_i].
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sampler as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0.2


def _agent(**kw):
    from marlmaze.PPO import PPO

    for k, v in dict(load=False, verbose=False, save=False, device="cpu").items():
        kw.setdefault(k, v)
    return PPO(2, **kw)


def entropy64(z, mk):
    """H_move + H_mark per agent row in numpy fp64 (module doc): z [R, 6], mk [R, 6] bool."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(mk[:, :5], z[:, :5], -np.inf)
        mx = m.max(1, keepdims=True)
        e = np.where(mk[:, :5], np.exp(m - mx), 0.0)
        se = e.sum(1, keepdims=True)
        p = e / se
        logp = (m - mx) - np.log(se)
        h_move = -np.where(p > 0, p * logp, 0.0).sum(1)
    h_move = np.where(mk[:, :5].any(1), h_move, 0.0)
    a = np.abs(z[:, 5])
    t = np.exp(-a)
    h_mark = np.where(mk[:, 5], np.log1p(t) + a * t / (1 + t), 0.0)
    return h_move + h_mark


@pytest.fixture(scope="module")
def batch(golden):
    """The 256-sample fixture with old log-probs moved off the current policy's (ratios on both sides of the clip
    range) and the agent's own logits for the closed forms."""
    fx = golden("nets")
    obs, act, adv, rtg, masks = (torch.as_tensor(fx[k]) for k in ("obs", "actions", "advs", "rtgs", "masks"))
    ag = _agent(diagnostics=True)
    with torch.no_grad():
        ml, kl = ag.actor(obs.reshape(-1, 65))
    z = torch.cat([ml, kl.reshape(-1, 1)], 1).numpy()
    mk = masks.reshape(-1, 6).numpy().astype(bool)
    lp = S.logp64(z[:, :5], z[:, 5], mk, act.reshape(-1, 2).numpy()).reshape(-1, 2).sum(1)
    noise = np.random.default_rng(5).normal(0, 0.3, lp.shape[0])
    old = torch.as_tensor((lp - noise).astype(np.float32))
    return dict(obs=obs, act=act, old=old, adv=adv, rtg=rtg, masks=masks, z=z, mk=mk, lp=lp)


def _actor_grads(ag):
    return {k: p.grad.detach().clone() for k, p in ag.actor.named_parameters()}


def test_host_stats_match_closed_forms(batch):
    b = batch
    ag = _agent(ent_coef=0.01)
    assert ag.stats_on and ag.last_update_stats is None
    st = torch.full((4,), float("nan"))
    ag.minibatch_grads(b["obs"], b["act"], b["old"], b["adv"], b["rtg"], b["masks"], stats_out=st)
    d = b["lp"] - b["old"].numpy().astype(np.float64)
    r = np.exp(d)
    edge = np.minimum(np.abs(r - (1 - CLIP)), np.abs(r - (1 + CLIP)))
    assert edge.min() >= 1e-4, edge.min()  # the clipped count does not depend on rounding
    out = (r < 1 - CLIP) | (r > 1 + CLIP)
    assert 0 < out.sum() < out.size
    ref = [entropy64(b["z"], b["mk"]).reshape(-1, 2).sum(1).mean(), (np.expm1(d) - d).mean(), out.mean(), r.max()]
    print("host stats", st.tolist(), "closed forms", ref)
    for got, want in zip(st.tolist(), ref):
        assert abs(got - want) <= 1e-5 * abs(want) + 1e-7, (st.tolist(), ref)
    assert ref[0] > 0 and ref[1] > 0


def test_host_entropy_gradient_scales_with_the_coefficient(batch):
    """adv = 0: the surrogate's gradient is 0, so the actor's .grad is -c grad(mean H): linear in c (c = 2^-6,
    so that the scaling is exact in fp32 and rtol 1e-5 is not a statement about rounding), nonzero in every
    tensor, and exactly zero without a bonus."""
    b = batch
    zero = torch.zeros_like(b["adv"])
    c = 2.0 ** -6
    grads = {}
    for coef in (1.0, c, 0.0):
        ag = _agent(ent_coef=coef, diagnostics=True)
        ag.minibatch_grads(b["obs"], b["act"], b["old"], zero, b["rtg"], b["masks"])
        grads[coef] = _actor_grads(ag)
    for k, g1 in grads[1.0].items():
        assert g1.abs().max() > 0, k
        np.testing.assert_allclose(grads[c][k].numpy(), c * g1.numpy(), rtol=1e-5, atol=0, err_msg=k)
        assert (grads[0.0][k] == 0).all(), k


def entropy_grad64(z, mk):
    """d (H_move + H_mark) / d z per agent row in numpy fp64: -p_j (log p_j + H_move) in a legal move column,
    -z_5 s (1 - s), s = sigmoid(z_5), in an allowed mark column, 0 in every masked column."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(mk[:, :5], z[:, :5], -np.inf)
        mx = m.max(1, keepdims=True)
        e = np.where(mk[:, :5], np.exp(m - mx), 0.0)
        se = e.sum(1, keepdims=True)
        p = e / se
        logp = np.where(p > 0, (m - mx) - np.log(se), 0.0)
        h = -(p * logp).sum(1, keepdims=True)
        gm = np.where(p > 0, -p * (logp + h), 0.0)
    gm[~mk[:, :5].any(1)] = 0.0
    s = 1.0 / (1.0 + np.exp(-z[:, 5]))
    gk = np.where(mk[:, 5], -z[:, 5] * s * (1 - s), 0.0)
    return np.concatenate([gm, gk[:, None]], 1)


def test_host_entropy_gradient_sign_and_size(batch):
    """adv = 0, ent_coef = c: the actor's .grad equals the closed-form head gradient -(c / M) dH/dz (fp64)
    pushed through the actor's own backward -- the sign of the bonus and its 1 / M factor.  Both sides run the
    trunk's backward in fp32 torch; 1e-4 of max |g| per tensor covers the fp32 head gradient of the host form."""
    b = batch
    c, M = 0.01, b["obs"].shape[0]
    ag = _agent(ent_coef=c)
    ag.minibatch_grads(b["obs"], b["act"], b["old"], torch.zeros_like(b["adv"]), b["rtg"], b["masks"])
    got = _actor_grads(ag)
    ag.actor_optim.zero_grad(set_to_none=True)
    ml, kl = ag.actor(b["obs"].reshape(-1, 65))
    dz = torch.as_tensor(-(c / M) * entropy_grad64(b["z"], b["mk"]), dtype=torch.float32)
    torch.cat([ml, kl.reshape(-1, 1)], 1).backward(dz)
    for k, p in ag.actor.named_parameters():
        scale = p.grad.abs().max().item()
        assert scale > 0, k
        assert (got[k] - p.grad).abs().max().item() <= 1e-4 * scale, k


def test_default_agent_has_no_stats_and_todays_history_keys(batch):
    b = batch
    ag = _agent()
    assert not ag.stats_on and ag.ent_coef == 0.0 and ag.last_update_stats is None
    ag.minibatch_grads(b["obs"], b["act"], b["old"], b["adv"], b["rtg"], b["masks"])
    assert ag.last_update_stats is None
    with pytest.raises(ValueError):
        _agent(ent_coef=float("nan"))


def test_update_fills_last_update_stats_and_hist_keeps_its_meaning(golden):
    """PPO.update on the CPU: hist [K, 4] of an ent_coef = 0 diagnostics agent equals the default agent's bit for
    bit and so do the parameters; last_update_stats is [K, 4], finite, in range."""
    t = golden("train_small")
    B = 320
    args = [torch.as_tensor(t[k][:B]) for k in ("obs", "actions", "logp", "masks", "advs", "vals")]
    idx = np.random.default_rng(0).permutation(B)
    torch.set_num_threads(1)
    res = []
    for diag in (False, True):
        ag = _agent(batch_size=B, updates_per_batch=1, diagnostics=diag)
        hist = ag.update(*args, index_list=idx)
        res.append((hist, {k: v.clone() for k, v in ag.actor.state_dict().items()}, ag.last_update_stats))
    (h0, p0, s0), (h1, p1, s1) = res
    assert s0 is None and s1.shape == (5, 4) and s1.dtype == torch.float32
    assert torch.equal(h0, h1) and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert torch.isfinite(s1).all()
    assert (s1[:, 0] > 0).all() and (s1[:, 1] >= 0).all() and ((s1[:, 2] >= 0) & (s1[:, 2] <= 1)).all()
    assert (s1[:, 3] > 0).all()


_DP_WORKER = r"""
import os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {repo!r})
import numpy as np, torch
import torch.distributed as dist
from marlmaze.dist import DP
from marlmaze.PPO import PPO
rank, world = int(sys.argv[1]), 2
os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
dp = DP.from_env(backend="gloo")
torch.set_num_threads(1)
data = np.load(sys.argv[3])
Bl = data["obs"].shape[0] // world
sl = slice(rank * Bl, (rank + 1) * Bl)
local = []
reduce = dp.allreduce_update_stats
def keep_local(stats):  # this rank's values, before the collective
    local.append(stats.clone())
    return reduce(stats)
dp.allreduce_update_stats = keep_local
ag = PPO(2, batch_size=world * Bl, updates_per_batch=1, lr=1e-4, device="cpu", dp=dp, load=False, verbose=False,
         save=False, ent_coef=0.01)
ag.update(*(torch.as_tensor(data[k][sl]) for k in ("obs", "act", "logp", "masks", "adv", "val")),
          index_list=data["idx%d" % rank])
assert len(local) == 1
np.savez(sys.argv[4] + "_%d.npz" % rank, local=local[0].numpy(), stats=ag.last_update_stats.numpy())
dist.destroy_process_group()
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_reduce_the_stats(tmp_path, golden):
    """Two gloo ranks, each on its half of the batch: both end with the same last_update_stats; its entropy, KL
    and clipped-fraction columns are the means of the two ranks' local values, its ratio_max column their
    maximum."""
    t = golden("train_small")
    B = 320
    rng = np.random.default_rng(2)
    data = dict(obs=t["obs"][:B], act=t["actions"][:B], logp=t["logp"][:B] + rng.normal(0, 0.2, B).astype(np.float32),
                masks=t["masks"][:B], adv=t["advs"][:B], val=t["vals"][:B])
    fx = str(tmp_path / "dp_in.npz")
    np.savez(fx, idx0=rng.permutation(B // 2), idx1=rng.permutation(B // 2), **data)
    port = str(_free_port())
    out = str(tmp_path / "dp_out")
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_DP_WORKER.format(pkg=os.path.join(REPO, "marl-maze_amd"), repo=REPO))
    procs = [subprocess.Popen([sys.executable, script, str(r), port, fx, out]) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    got = [np.load(out + f"_{r}.npz") for r in range(2)]
    assert got[0]["stats"].shape == (5, 4) and np.isfinite(got[0]["stats"]).all()
    assert np.array_equal(got[0]["stats"], got[1]["stats"])
    l0, l1 = got[0]["local"], got[1]["local"]
    assert not np.array_equal(l0, l1)  # the shards differ, so the reduction is not a no-op
    np.testing.assert_allclose(got[0]["stats"][:, :3], (l0[:, :3] + l1[:, :3]) / 2, rtol=1e-6, atol=1e-9)
    assert np.array_equal(got[0]["stats"][:, 3], np.maximum(l0[:, 3], l1[:, 3]))
    assert (l0[:, 3] != l1[:, 3]).any()
