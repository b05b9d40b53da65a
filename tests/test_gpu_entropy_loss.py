"""mm_ppo_loss_ent / mm_ppo_loss_ent_bwd / mm_ppo_stats_final: the policy loss with an entropy bonus,
surrogate - c mean_i H_i, and the update's diagnostics [entropy, approx_kl, clip_frac, ratio_max], from the
kernels up to PPO.update.  The host (CPU torch) form and the data-parallel reduction: tests/test_cpu_entropy.py.

References are fp64 torch (torch.distributions for the entropies, torch.expm1(d) - d for the KL estimate,
autograd for the gradients).  The bar is tests/test_gpu_policy_loss_edges.py's: the kernel's error is at most
max(2 x the error of the same formula in fp32 torch on the GPU, floor), floors 1e-6 |value| + 1e-7 for a scalar
and 1e-6 max |g| for a gradient.
"""
import copy

import numpy as np
import pytest
import torch

import test_gpu_policy_loss_edges as E
import test_gpu_update_parity as P
from oracle import ppo as oppo
from oracle import sampler as S

pytestmark = pytest.mark.gpu

M = E.M  # 517: two full 256-sample workgroups and a ragged tail of 5; the backward runs 1,034 rows
CLIP = 0.2
CLASSES = E.CLASSES + ["uniform", "saturated"]
ENT, KL, CLIPFRAC, RATIO_MAX = 0, 1, 2, 3
SAT_MARK = 40.0


def _samples(clip=CLIP):
    """As test_gpu_policy_loss_edges._samples (one class per sample, every branch of the surrogate taken by
    design), with two more classes:

    * uniform: equal move logits over the legal set, so H_move = log n_legal;
    * saturated: move logits x 30 (the softmax of the others underflows to 0 in fp32 wherever the gap to the
      maximum passes 104) and the mark logit x 30, limited to |z_5| <= 40: past |z_5| = 88 every fp32 evaluation
      of s (1 - s) is 0 (exp(-88) is fp32's smallest normal), and the test demands a nonzero column 5 of every
      row whose mark is allowed.  (test_huge_logits_stay_finite runs |z| up to 300 without that demand.)

    and the rows of above_pos / above_neg scaled by 0.25 like first_epoch's: the largest ratio is theirs, a
    ratio's relative error is the absolute error of logp, i.e. about an ulp of |logp|, and ratio_max is held to
    1e-6: |logp| < 8 keeps an ulp below 4.8e-7.  Returns the arrays of E._samples."""
    rng = np.random.default_rng(517)
    z = rng.normal(0, 2, (2 * M, 6)).astype(np.float32)
    mk = rng.random((2 * M, 6)) < 0.7
    mk[:, 4] = True  # stay is always legal
    cls = np.arange(M) % len(CLASSES)
    rows = np.repeat(cls, 2)
    ix = CLASSES.index
    for name in ("first_epoch", "above_pos", "above_neg"):
        z[rows == ix(name)] *= 0.25
    mk[rows == ix("mark_disallowed"), 5] = False
    single = rows == ix("single_legal")
    mk[single, :5] = False
    mk[np.nonzero(single)[0], rng.integers(0, 5, single.sum())] = True
    mk[single, 5] = True
    uni = rows == ix("uniform")
    z[uni, :5] = z[uni, 0:1]
    sat = rows == ix("saturated")
    z[sat, :5] *= 30
    z[sat, 5] = np.clip(z[sat, 5] * 30, -SAT_MARK, SAT_MARK)
    move = np.where(mk[:, :5], rng.random((2 * M, 5)), -1.0).argmax(1)  # a legal move, uniformly
    mark = (rng.random(2 * M) < 0.5) & mk[:, 5]
    # (saturated rows take the likelier mark: fp32's 1 - sigmoid(z_5) is 0 from z_5 = 17 on, and the log-prob of
    # the other mark -inf, in mm_ppo_loss and in torch alike)
    mark[sat] = (z[sat, 5] > 0) & mk[sat, 5]
    act = np.stack([move, mark.astype(np.int64)], 1)
    lp64 = S.logp64(z[:, :5], z[:, 5], mk, act).reshape(M, 2).sum(1)
    want =np.exp(rng.uniform(-0.05, 0.05, M))
    want[cls == ix("first_epoch")] = np.exp(rng.uniform(-4e-7, 4e-7, (cls == ix("first_epoch")).sum()))
    for name, r in (("below_pos", 0.5 * (1 - clip)), ("below_neg", 0.5 * (1 - clip)), ("above_pos", 2 * (1 + clip)),
                    ("above_neg", 2 * (1 + clip))):
        want[cls == ix(name)] = r
    old = (lp64 - np.log(want)).astype(np.float32)
    adv = rng.normal(0, 1, M)
    adv = np.where(np.abs(adv) < 0.05, 0.05, adv)
    for name, sign in (("below_pos", 1), ("below_neg", -1), ("above_pos", 1), ("above_neg", -1)):
        c = cls == ix(name)
        adv[c] = sign * np.abs(adv[c])
    adv[cls == ix("zero_adv")] = 0.0
    ratio = np.exp(lp64 - old.astype(np.float64))
    return z, mk, act, old, adv.astype(np.float32), cls, ratio


def torch_terms(heads, masks, act, old_lp, A, clip):
    """(surrogate loss, mean joint entropy, mean KL estimate, ratios) of heads [2m, 6] in heads' dtype."""
    m = old_lp.shape[0]
    ml = heads[:, :5].masked_fill(~masks[:, :5], float("-inf"))
    lp = torch.log_softmax(ml, -1).gather(1, act[:, 0:1]).squeeze(1)
    kl = heads[:, 5].masked_fill(~masks[:, 5], float("-inf"))
    p = torch.sigmoid(kl)
    p = torch.where(act[:, 1] != 0, p, 1 - p)
    d = (lp + torch.log(p)).view(m, 2).sum(1) - old_lp
    r = torch.exp(d)
    surr = -torch.mean(torch.min(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A))
    h_move = torch.distributions.Categorical(logits=ml).entropy()
    z5 = torch.where(masks[:, 5], heads[:, 5], torch.zeros_like(heads[:, 5]))
    h_mark = torch.where(masks[:, 5], torch.distributions.Bernoulli(logits=z5).entropy(), torch.zeros_like(z5))
    H = (h_move + h_mark).view(m, 2).sum(1).mean()
    return surr, H, (torch.expm1(d) - d).mean(), r


def _torch_ref(dz, dmasks, dact, dold, dadv, clip, cs, dtype):
    """Scalars and, per coefficient c, d (surrogate - c H) / d heads by autograd, in ``dtype``."""
    z = dz.detach().clone().to(dtype).requires_grad_(True)
    surr, H, kl, r = torch_terms(z, dmasks, dact, dold.to(dtype), dadv.to(dtype), clip)
    grads = {c: torch.autograd.grad(surr - c * H, z, retain_graph=True)[0] for c in cs}
    return dict(surr=surr.item(), ent=H.item(), kl=kl.item(), rmax=r.max().item(), grads=grads)


def _kernel(dz, dmasks, dact, dold, dadv, clip, c):
    """The three kernels on heads dz: (stats [4], surrogate loss, dheads)."""
    from marlmaze import update
    from marlmaze.PPO import _ppo_loss_ent_bwd, _ppo_loss_ent_fwd, _u8

    m = dold.shape[0]
    mk, a8 = _u8(dmasks), dact.to(torch.int8).contiguous()
    coef, part, spart = _ppo_loss_ent_fwd(dz, mk, a8, dold, dadv, clip, c)
    stats = update.ppo_stats_final(spart, m, torch.full((4,), float("nan"), device=dz.device))
    one = torch.ones(1, device=dz.device)
    return stats, -part.sum() / m, _ppo_loss_ent_bwd(dz, mk, a8, coef, one, c), (coef, part, spart)


def _scalar_ok(got, ref, ref32, what):
    e_ours, e_torch = abs(got - ref), abs(ref32 - ref)
    print(f"{what}: {ref:.9g}: |kernel - fp64| {e_ours:.3g}, |torch fp32 - fp64| {e_torch:.3g}")
    assert e_ours <= max(2.0 * e_torch, 1e-6 * abs(ref) + 1e-7), (what, got, ref, e_ours, e_torch)


def _check(arrays, clip, tag, demand_mark_column=True):
    """Stats and gradients of one set of samples against fp64; the exact zeros."""
    z, mk, act, old, adv, ratio = arrays
    m = old.shape[0]
    edge = np.minimum(np.abs(ratio - (1 - clip)), np.abs(ratio - (1 + clip)))
    assert edge.min() >= 1e-4, edge.min()  # no sample's side of a clip edge depends on rounding
    n_out = int(((ratio < 1 - clip) | (ratio > 1 + clip)).sum())
    dz, dmasks, dact, dold, dadv = (torch.as_tensor(x).cuda() for x in (z, mk, act, old, adv))
    cs = (0.01, 1.0)
    r64 = _torch_ref(dz, dmasks, dact, dold, dadv, clip, cs, torch.float64)
    r32 = _torch_ref(dz, dmasks, dact, dold, dadv, clip, cs, torch.float32)
    for c in cs:
        stats, surr, got, _ = _kernel(dz, dmasks, dact, dold, dadv, clip, c)
        st = stats.tolist()
        assert np.isfinite(st).all() and torch.isfinite(got).all()
        _scalar_ok(surr.item(), r64["surr"], r32["surr"], f"{tag} c={c} surrogate")
        _scalar_ok(st[ENT], r64["ent"], r32["ent"], f"{tag} c={c} entropy")
        _scalar_ok(st[KL], r64["kl"], r32["kl"], f"{tag} c={c} approx_kl")
        print(f"{tag} c={c}: clip_frac {st[CLIPFRAC]!r} (reference {n_out} / {m}), ratio_max {st[RATIO_MAX]!r} "
              f"(reference {r64['rmax']!r})")
        assert st[CLIPFRAC] == float(np.float32(n_out / m)), (st[CLIPFRAC], n_out, m)
        assert abs(st[RATIO_MAX] - r64["rmax"]) <= 1e-6 * r64["rmax"], (st[RATIO_MAX], r64["rmax"])
        g64 = r64["grads"][c]
        ge_ours = (got.double() - g64).abs().max().item()
        ge_torch = (r32["grads"][c].double() - g64).abs().max().item()
        gmax = g64.abs().max().item()
        print(f"{tag} c={c}: max |g| {gmax:.3g}: |kernel - fp64| {ge_ours:.3g}, |torch fp32 - fp64| {ge_torch:.3g}")
        assert ge_ours <= max(2.0 * ge_torch, 1e-6 * gmax), (tag, c, ge_ours, ge_torch, gmax)
        # exact zeros of the total gradient
        g = got.cpu().numpy()
        assert (g[:, :5][~mk[:, :5]] == 0).all()
        assert (g[~mk[:, 5], 5] == 0).all()
        one = mk[:, :5].sum(1) == 1
        assert (g[one, :5] == 0).all()
        if c == 1.0 and demand_mark_column:  # the zeros above are not a kernel that writes nothing
            live = mk[:, 5] & (z[:, 5] != 0)
            assert live.sum() > 0 and (g[live, 5] != 0).all()
    return r64


@pytest.fixture(scope="module")
def samples():
    return _samples()


def test_kernel_values_and_gradient_by_class(samples):
    """M = 517 samples in eleven classes (_samples): the four statistics and d (surrogate - c mean H) / d heads at
    c = 0.01 and c = 1 (the entropy part dominates) against fp64 torch; clip_frac equals the fp64 count / M
    exactly; exact zeros in illegal move columns, in column 5 where the mark is disallowed and in all five move
    columns of single-legal-move rows; column 5 nonzero wherever the mark is allowed."""
    z, mk, act, old, adv, cls, ratio = samples
    is_ = lambda name: cls == CLASSES.index(name)  # noqa: E731
    rows = np.repeat(cls, 2)
    assert all(is_(c).sum() >= 47 for c in CLASSES)
    assert (~mk[:, 5]).sum() >= 2 * 47 and (mk[:, :5].sum(1) == 1).sum() >= 2 * 47
    # the classes are what they claim: uniform rows have H_move = log n_legal, saturated rows underflow in fp32
    uni = rows == CLASSES.index("uniform")
    p, _ = S.probs64(z[uni, :5], z[uni, 5], mk[uni])
    n_legal = mk[uni, :5].sum(1)
    h_uni = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(1)
    assert np.abs(h_uni - np.log(n_legal)).max() <= 1e-12 and (n_legal > 1).any()
    sat = rows == CLASSES.index("saturated")
    zs = np.where(mk[sat, :5], z[sat, :5], -np.inf)
    gap = zs.max(1, keepdims=True) - zs
    assert ((gap > 104) & np.isfinite(gap)).any(1).sum() >= 10  # expf(-104) == 0 in fp32
    assert np.abs(z[sat, 5]).max() == SAT_MARK
    r64 = _check((z, mk, act, old, adv, ratio), CLIP, "M=517")
    assert 0.15 < r64["ent"] / 2 < np.log(5) + np.log(2)


def test_one_sample(samples):
    """M = 1 (one workgroup with one live thread, two backward rows): the same checks."""
    z, mk, act, old, adv, cls, ratio = samples
    i = CLASSES.index("inside")
    assert mk[2 * i:2 * i + 2, 5].any()
    _check((z[2 * i:2 * i + 2], mk[2 * i:2 * i + 2], act[2 * i:2 * i + 2], old[i:i + 1], adv[i:i + 1],
            ratio[i:i + 1]), CLIP, "M=1", demand_mark_column=mk[2 * i:2 * i + 2, 5].any())


def test_huge_logits_stay_finite():
    """Rows with |z| up to about 300 (move and mark logits x 100): every statistic and every gradient entry is
    finite and within the bar of fp64; where exp(-|z_5|) underflows the entropy gradient of column 5 is 0."""
    rng = np.random.default_rng(3)
    m = 64
    z = (rng.normal(0, 1, (2 * m, 6)) * 100).astype(np.float32)
    mk = rng.random((2 * m, 6)) < 0.7
    mk[:, 4] = True
    # the likeliest action of every row: |logp| stays small, so the fp32 ratios are as accurate as elsewhere
    move = np.where(mk[:, :5], z[:, :5], -np.inf).argmax(1)
    mark = (z[:, 5] > 0) & mk[:, 5]
    act = np.stack([move, mark.astype(np.int64)], 1)
    lp64 = S.logp64(z[:, :5], z[:, 5], mk, act).reshape(m, 2).sum(1)
    old = (lp64 - rng.uniform(-0.05, 0.05, m)).astype(np.float32)
    adv = rng.normal(0, 1, m).astype(np.float32)
    ratio = np.exp(lp64 - old.astype(np.float64))
    assert np.abs(z).max() > 250
    _check((z, mk, act, old, adv, ratio), CLIP, "huge", demand_mark_column=False)
    dz, dmasks, dact, dold = (torch.as_tensor(x).cuda() for x in (z, mk, act, old))
    _, _, got, _ = _kernel(dz, dmasks, dact, dold, torch.zeros(m, device="cuda"), CLIP, 1.0)
    under = mk[:, 5] & (np.abs(z[:, 5]) > 110)
    assert under.sum() > 0 and (got.cpu().numpy()[under, 5] == 0).all()


def test_zero_coefficient_changes_nothing_and_runs_repeat(samples):
    """mm_ppo_loss_ent(ent_coef = 0) gives mm_ppo_loss's coef and partial, mm_ppo_loss_ent_bwd(ent_coef = 0)
    gives mm_ppo_loss_bwd's dheads (torch.equal), also with dloss != 1; the forward's outputs do not depend on
    the coefficient; two runs of every new kernel are bitwise equal."""
    from marlmaze import update
    from marlmaze.PPO import _ppo_loss_bwd, _ppo_loss_ent_bwd, _ppo_loss_ent_fwd, _ppo_loss_fwd, _u8

    z, mk, act, old, adv, cls, ratio = samples
    dz, dold, dadv = (torch.as_tensor(x).cuda() for x in (z, old, adv))
    dmk, a8 = _u8(torch.as_tensor(mk).cuda()), torch.as_tensor(act).to(torch.int8).cuda()
    coef0, part0 = _ppo_loss_fwd(dz, dmk, a8, dold, dadv, CLIP)
    for dloss in (1.0, 0.37):
        dl = torch.full((1,), dloss, device="cuda")
        g0 = _ppo_loss_bwd(dz, dmk, a8, coef0, dl)
        assert torch.equal(_ppo_loss_ent_bwd(dz, dmk, a8, coef0, dl, 0.0), g0)
    runs = []
    for c in (0.0, 0.0, 0.01, 0.01):
        coef, part, spart = _ppo_loss_ent_fwd(dz, dmk, a8, dold, dadv, CLIP, c)
        assert torch.equal(coef, coef0) and torch.equal(part, part0)
        stats = update.ppo_stats_final(spart, M, torch.empty(4, device="cuda"))
        g = _ppo_loss_ent_bwd(dz, dmk, a8, coef, torch.ones(1, device="cuda"), c)
        runs.append((coef, part, spart, stats, g))
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(runs[0][:4], runs[2][:4]))
    assert not torch.equal(runs[0][4], runs[2][4])


@pytest.mark.parametrize("n", [1, 1034 * 6, 300007])
def test_pow2_norm_and_scale_by(n):
    """mm_pow2_norm / mm_scale_by (the range normalisation of dz with an entropy bonus): kappa is a power of two
    with kappa max|x| target in [1, 2), its inverse beside it; 1 for an all-zero or non-finite x; NaN entries do
    not count; scaling by kappa and by 1 / kappa gives x back bit for bit.  n = 1, a ragged count, and one that
    takes every workgroup through its stride loop."""
    from marlmaze import update

    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, device="cuda", generator=g) * 3e-7
    target = 517 / 4.0
    k = update.pow2_norm(x, target)
    kap, inv = k.tolist()
    m = x.abs().max().item()
    assert 1.0 <= kap * m * target < 2.0 and np.log2(kap) == round(np.log2(kap)) and kap * inv == 1.0
    y = update.scale_by(x.clone(), k[0:1])
    assert torch.equal(y, x * kap)
    assert torch.equal(update.scale_by(y, k[1:2]).view(torch.int32), x.view(torch.int32))
    assert update.pow2_norm(torch.zeros(n, device="cuda"), target).tolist() == [1.0, 1.0]
    bad = x.clone()
    bad[n // 2] = float("inf")
    assert update.pow2_norm(bad, target).tolist() == [1.0, 1.0]
    if n > 1:
        bad[n // 2] = float("nan")
        assert update.pow2_norm(bad, target).tolist() == update.pow2_norm(torch.cat([x[:n // 2], x[n // 2 + 1:]]),
                                                                          target).tolist()


# ---- through the networks ----
def _check_grads(got, ref, tag, ref32=None, rel=1e-5):
    """test_gpu_update_parity._check_grads's rule.  Per tensor: max|g - g64| <= rel max|g64|, or -- for a tensor
    on which the reference's own fp32 arithmetic (ref32) is further than that from g64 -- no further from g64 than
    twice the reference's own error."""
    assert set(got) == set(ref)
    bad = []
    for k in ref:
        r = ref[k].double()
        scale = r.abs().max().item()
        err = (got[k].double() - r).abs().max().item()
        bound, err32 = rel * scale, float("nan")
        if ref32 is not None:
            err32 = (ref32[k].double() - r).abs().max().item()
            bound = max(bound, 2.0 * err32)
        if err > rel * scale:
            print(f"{tag} {k}: err {err / scale:.2e} of max|g|, fp32 oracle {err32 / scale:.2e}")
        if err > bound + 1e-12:
            bad.append((k, err / scale))
    assert not bad, (tag, bad)


def _oracle_actor_grads(actor, obs, act, old_lp, adv, masks, c, clip=CLIP, pa=None):
    """Autograd of surrogate - c mean H through the oracle actor (oracle.ppo.OActor, fp32 or fp64), the
    surrogate as oracle.ppo.minibatch_grads writes it.  pa: the actor's ReLU patterns (OActor.forward)."""
    dt = next(actor.parameters()).dtype
    obs, adv, old_lp = (t.to(dt) for t in (obs, adv, old_lp))
    cur, H = 0, 0
    for i in range(2):
        ml, kl = actor(obs[:, i, :]) if pa is None else actor(obs[:, i, :], [m[i::2] for m in pa])
        mk = masks[:, i]
        ml = ml.masked_fill(~mk[:, 0:5], float("-inf"))
        cat = torch.distributions.Categorical(logits=ml)
        kl = kl.squeeze(1)
        p = torch.sigmoid(kl.masked_fill(~mk[:, 5], float("-inf")))
        p = torch.where(act[:, i, 1].to(torch.bool), p, 1 - p)
        cur = cur + cat.log_prob(act[:, i, 0]) + torch.log(p)
        z5 = torch.where(mk[:, 5], kl, torch.zeros_like(kl))
        H = H + cat.entropy() + torch.where(mk[:, 5], torch.distributions.Bernoulli(logits=z5).entropy(),
                                            torch.zeros_like(kl))
    ratio = torch.exp(cur - old_lp)
    surr = -torch.mean(torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv))
    g = torch.autograd.grad(surr - c * H.mean(), list(actor.parameters()))
    return {k: v for (k, _), v in zip(actor.named_parameters(), g)}


@pytest.fixture(scope="module")
def nets_case(golden):
    """The 256-sample fixture, the oracle networks, a default agent's gradients on it (for the critic) and the GPU
    forward's ReLU patterns."""
    fx = golden("nets")
    actor, critic = P._oracle_nets(fx)
    batch = P._minibatch(fx, 256)
    ag0 = P._agent(n_envs=64)
    P._to_gpu(ag0, actor, critic)
    actor64, critic64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    (pa, _), flips = P._patterns(ag0, batch, actor64, critic64)
    ag0.minibatch_grads(*(t.cuda() for t in batch))
    _, gc0 = P._gpu_grads(ag0)
    return dict(actor=actor, critic=critic, actor64=actor64, batch=batch, pa=pa, flips=flips, gc0=gc0)


@pytest.mark.parametrize("zero_adv", [False, True])
def test_actor_gradients_through_the_networks(nets_case, zero_adv):
    """minibatch_grads of an ent_coef = 0.01 agent on the fixture: the per-tensor actor gradients against fp64
    autograd of surrogate - c mean H through the oracle actor (at the GPU forward's ReLU pattern, as
    test_gpu_update_parity), under _check_grads's rule; the critic's gradients equal the ent_coef = 0 agent's bit
    for bit; the actor loss stays the surrogate.  zero_adv: the whole actor gradient is -c grad(mean H), nonzero
    in every tensor -- the case that fails if the bonus's sign or its 1 / M factor is wrong."""
    n, c = nets_case, 0.01
    obs, act, old, adv, rtg, masks = n["batch"]
    if zero_adv:
        adv = torch.zeros_like(adv)
    act_l = act.long()
    ref = _oracle_actor_grads(n["actor64"], obs, act_l, old, adv, masks, c, pa=n["pa"])
    ref32 = _oracle_actor_grads(n["actor"], obs, act_l, old, adv, masks, c)
    if n["flips"]:  # the fp32 oracle's own error is measured against fp64 at its own pattern
        own = _oracle_actor_grads(n["actor64"], obs, act_l, old, adv, masks, c)
        ref32 = {k: v - own[k] + ref[k] for k, v in ref32.items()}
    ag = P._agent(n_envs=64, ent_coef=c)
    P._to_gpu(ag, n["actor"], n["critic"])
    st = torch.full((4,), float("nan"), device="cuda")
    al, _ = ag.minibatch_grads(*(t.cuda() for t in (obs, act, old, adv, rtg, masks)), stats_out=st)
    ga, gc = P._gpu_grads(ag)
    tag = f"ent_coef {c}, adv {'0' if zero_adv else 'fixture'}"
    _check_grads(ga, ref, tag, ref32)
    assert all(torch.equal(gc[k], n["gc0"][k]) for k in gc)
    assert torch.isfinite(st).all() and st[ENT] > 0
    if zero_adv:
        assert float(al) == 0.0
        for k, g in ga.items():
            assert g.abs().max().item() > 0, k
    else:
        ra, *_ = oppo.minibatch_grads(n["actor"], n["critic"], obs, act, old, adv, rtg, masks)
        assert abs(float(al) - ra) <= 1e-5 * abs(ra) + 1e-6, (float(al), ra)


# ---- PPO.update / PPO.train ----
def test_diagnostics_without_a_bonus_are_invisible(golden):
    """One update on the fixture batch with the same index_list: flat.data, both Adam moments and hist of a
    diagnostics=True, ent_coef=0 agent equal a default agent's (torch.equal); its last_update_stats is [K, 4],
    finite and in range; the default agent has none."""
    fx = golden("nets")
    obs, act, old, adv, rtg, masks = (t.cuda() for t in P._minibatch(fx, 256))
    res = []
    for diag in (False, True):
        ag = P._agent(n_envs=64, batch_size=256, sample_seed=7, diagnostics=diag)
        hist = ag.update(obs, act, old, masks, adv, rtg - adv, index_list=torch.arange(256))
        torch.cuda.synchronize()
        assert not ag.last_update_discarded and ag.range_redos == 0
        res.append((ag, hist))
    (a0, h0), (a1, h1) = res
    assert a0.last_update_stats is None and not a0.stats_on and a1.stats_on
    assert torch.equal(h0, h1) and torch.equal(a0.flat.data, a1.flat.data)
    assert torch.equal(a0.actor_optim.exp_avg, a1.actor_optim.exp_avg)
    assert torch.equal(a0.actor_optim.exp_avg_sq, a1.actor_optim.exp_avg_sq)
    assert torch.equal(a0.critic_optim.exp_avg, a1.critic_optim.exp_avg)
    assert torch.equal(a0.critic_optim.exp_avg_sq, a1.critic_optim.exp_avg_sq)
    st = a1.last_update_stats
    assert st.shape == (h1.shape[0], 4) and st.dtype == torch.float32 and st.is_cuda
    assert torch.isfinite(st).all()
    assert ((st[:, CLIPFRAC] >= 0) & (st[:, CLIPFRAC] <= 1)).all() and (st[:, KL] >= 0).all()
    assert (st[:, ENT] > 0).all() and (st[:, RATIO_MAX] > 0).all()


def test_train_history_keys():
    """A default agent's history entries have today's keys only; with stats on they gain entropy, approx_kl,
    clip_frac and ratio_max (the last minibatch's)."""
    n, T = 64, 16
    kw = dict(n_envs=n, horizon=T, batch_size=n * T, epochs=1, sample_seed=9, bootstrap=False,
              env_config=dict(default_size=(10, 10), max_timestep=40, seed_base=0))
    base = {"epoch", "episodes", "mean_len", "mean_shortest", "actor_loss", "critic_loss"}
    ag = P._agent(**kw)
    ag.train()
    assert ag.last_update_stats is None and set(ag.history[-1]) == base
    bg = P._agent(ent_coef=0.01, **kw)
    bg.train()
    h = bg.history[-1]
    assert set(h) == base | {"entropy", "approx_kl", "clip_frac", "ratio_max"}
    assert [h[k] for k in ("entropy", "approx_kl", "clip_frac", "ratio_max")] == bg.last_update_stats[-1].tolist()
    assert np.isfinite([h[k] for k in h]).all() and h["entropy"] > 0 and 0 <= h["clip_frac"] <= 1
