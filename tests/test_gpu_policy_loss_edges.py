"""mm_ppo_loss / mm_ppo_loss_bwd at the edges of the clipped surrogate (PPO.py:62-72), with samples built by
class so that every branch is taken by design and none by accident of a random draw."""
import numpy as np
import pytest
import torch

from oracle import sampler as S

pytestmark = pytest.mark.gpu

M = 517  # two full 256-sample workgroups and a ragged tail of 5
CLASSES = ["first_epoch", "below_pos", "below_neg", "above_pos", "above_neg", "zero_adv", "mark_disallowed",
           "single_legal", "inside"]


def _samples(clip):
    """heads [2M, 6] f32, masks [2M, 6] bool, act [2M, 2], old_logp [M] f32, adv [M] f32, cls [M] (index into
    CLASSES), ratio [M] f64 (exp(logp64 - old_logp) of the arrays as the kernel gets them)."""
    rng = np.random.default_rng(517)
    z = rng.normal(0, 2, (2 * M, 6)).astype(np.float32)
    mk = rng.random((2 * M, 6)) < 0.7
    mk[:, 4] = True  # stay is always legal (maze_agent.py:136)
    cls = np.arange(M) % len(CLASSES)
    rows = np.repeat(cls, 2)  # the class of each agent row
    z[rows == CLASSES.index("first_epoch")] *= 0.25  # |logp| < 8: old_logp's fp32 rounding stays below 2.4e-7
    mk[rows == CLASSES.index("mark_disallowed"), 5] = False
    single = rows == CLASSES.index("single_legal")
    mk[single, :5] = False
    mk[np.nonzero(single)[0], rng.integers(0, 5, single.sum())] = True
    mk[single, 5] = True
    move = np.where(mk[:, :5], rng.random((2 * M, 5)), -1.0).argmax(1)  # a legal move, uniformly
    mark = (rng.random(2 * M) < 0.5) & mk[:, 5]
    act = np.stack([move, mark.astype(np.int64)], 1)
    lp64 = S.logp64(z[:, :5], z[:, 5], mk, act).reshape(M, 2).sum(1)
    # old_logp = logp - log(ratio wanted)
    want = np.exp(rng.uniform(-0.05, 0.05, M))  # inside every clip range used (log 0.9 = -0.105, log 1.1 = 0.095)
    want[cls == CLASSES.index("first_epoch")] = np.exp(rng.uniform(-4e-7, 4e-7, (cls == 0).sum()))
    for name, r in (("below_pos", 0.5 * (1 - clip)), ("below_neg", 0.5 * (1 - clip)), ("above_pos", 2 * (1 + clip)),
                    ("above_neg", 2 * (1 + clip))):
        want[cls == CLASSES.index(name)] = r
    old = (lp64 - np.log(want)).astype(np.float32)
    adv = rng.normal(0, 1, M)
    adv = np.where(np.abs(adv) < 0.05, 0.05, adv)
    for name, sign in (("below_pos", 1), ("below_neg", -1), ("above_pos", 1), ("above_neg", -1)):
        c = cls == CLASSES.index(name)
        adv[c] = sign * np.abs(adv[c])
    adv[cls == CLASSES.index("zero_adv")] = 0.0
    ratio = np.exp(lp64 - old.astype(np.float64))
    return z, mk, act, old, adv.astype(np.float32), cls, ratio


@pytest.mark.parametrize("clip", [0.1, 0.2, 0.3])
def test_policy_loss_branches_by_class(clip):
    """M = 517 samples in nine classes: ratio within 1e-6 of 1 (the first epoch: the tie of min()), ratio far
    below 1 - clip and far above 1 + clip with A > 0 and with A < 0, A == 0, rows with the mark disallowed, rows
    with a single legal move, ratios inside the range.  No ratio is within 1e-4 of a clip edge (asserted in fp64),
    so no sample's branch depends on rounding.

    * d loss / d heads is exactly 0 for the two clipped-away quadrants (below with A < 0, above with A > 0) and
      for A == 0 -- fails if the clamp's gradient leaks or a quadrant is exchanged; in illegal move columns; in
      column 5 where the mark is disallowed; in all five move columns of a single-legal-move row;
    * the loss and the gradient against the torch formula in fp64: the kernel's error is at most twice that of the
      same formula in fp32 on the GPU, with the floors 1e-6 |loss| + 1e-7 and 1e-6 max |g|."""
    from marlmaze.PPO import _PolicyLoss

    z, mk, act, old, adv, cls, ratio = _samples(clip)
    # the classes are what they claim, in fp64, on the fp32 arrays the kernel gets
    edge = np.minimum(np.abs(ratio - (1 - clip)), np.abs(ratio - (1 + clip)))
    assert edge.min() >= 1e-4, edge.min()
    is_ = lambda name: cls == CLASSES.index(name)  # noqa: E731
    assert np.abs(ratio[is_("first_epoch")] - 1).max() <= 1e-6
    below, above = is_("below_pos") | is_("below_neg"), is_("above_pos") | is_("above_neg")
    assert (ratio[below] < 0.6 * (1 - clip)).all() and (ratio[above] > 1.9 * (1 + clip)).all()
    assert ((ratio[~below & ~above] > 1 - clip) & (ratio[~below & ~above] < 1 + clip)).all()
    assert (adv[is_("below_pos") | is_("above_pos")] > 0).all() and (adv[is_("below_neg") | is_("above_neg")] < 0).all()
    assert (adv[is_("zero_adv")] == 0).all() and (adv[~is_("zero_adv")] != 0).all()
    assert all(is_(c).sum() >= 57 for c in CLASSES)

    dmasks = torch.as_tensor(mk).cuda()
    dact = torch.as_tensor(act).cuda()

    def torch_loss(heads, old_lp, A):  # tests/test_gpu_ppo.py::test_fused_policy_loss_matches_torch's formula
        ml = heads[:, :5].masked_fill(~dmasks[:, :5], float("-inf"))
        lp = torch.log_softmax(ml, -1).gather(1, dact[:, 0:1]).squeeze(1)
        kl = heads[:, 5].masked_fill(~dmasks[:, 5], float("-inf"))
        p = torch.sigmoid(kl)
        p = torch.where(dact[:, 1] != 0, p, 1 - p)
        cur = (lp + torch.log(p)).view(M, 2).sum(1)
        r = torch.exp(cur - old_lp)
        return -torch.mean(torch.min(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A))

    dz, dold, dadv = (torch.as_tensor(x).cuda() for x in (z, old, adv))
    z64 = dz.double().requires_grad_(True)
    ref = torch_loss(z64, dold.double(), dadv.double())
    g64, = torch.autograd.grad(ref, z64)
    z32 = dz.clone().requires_grad_(True)
    l32 = torch_loss(z32, dold, dadv)
    g32, = torch.autograd.grad(l32, z32)
    zk = dz.clone().requires_grad_(True)
    loss = _PolicyLoss.apply(zk, dmasks, dact.to(torch.int8), dold, dadv, clip)
    got, = torch.autograd.grad(loss, zk)

    # exact zeros
    g = got.cpu().numpy()
    rows = np.repeat(cls, 2)
    dead = np.isin(rows, [CLASSES.index(c) for c in ("below_neg", "above_pos", "zero_adv")])
    assert (g[dead] == 0).all()
    assert (g64.cpu().numpy()[dead] == 0).all()  # and so says the reference
    assert (g[:, :5][~mk[:, :5]] == 0).all()
    assert (g[~mk[:, 5], 5] == 0).all() and (~mk[:, 5]).sum() >= 2 * 57
    one = mk[:, :5].sum(1) == 1
    assert one.sum() >= 2 * 57 and (g[one, :5] == 0).all()
    live = ~dead & mk[:, 5]
    assert (g[live, 5] != 0).all()  # the zeros above are not a kernel that writes nothing

    e_ours, e_torch = abs(loss.item() - ref.item()), abs(l32.item() - ref.item())
    print(f"clip {clip}: loss {ref.item():.9g}: |kernel - fp64| {e_ours:.3g}, |torch fp32 - fp64| {e_torch:.3g}")
    ge_ours = (got.double() - g64).abs().max().item()
    ge_torch = (g32.double() - g64).abs().max().item()
    gmax = g64.abs().max().item()
    print(f"clip {clip}: max |g| {gmax:.3g}: |kernel - fp64| {ge_ours:.3g}, |torch fp32 - fp64| {ge_torch:.3g}")
    assert e_ours <= max(2.0 * e_torch, 1e-6 * abs(ref.item()) + 1e-7), (e_ours, e_torch)
    assert ge_ours <= max(2.0 * ge_torch, 1e-6 * gmax), (ge_ours, ge_torch)
