"""The per-row part of the update's critic as one launch (mm_critic_update, Critic.train_update_fused) against
the separate launches it replaces (the three forward GEMMs, mm_mse_loss's dV, mm_x3_heads_bwd and the
input-gradient GEMM of Critic.train_forward / train_backward) and the fp64 oracle.

* forward: V equals the unfused x2 forward bit for bit (the fused kernel repeats k_bres's fragments, k order
  and MFMA sequence), so the ReLU patterns the parity suite takes from train_forward are the fused step's;
* loss: mm_mse_loss on the same V: equal (the bound of fp32 rounding of the sum, 128 * 2^-24 of the loss for
  the under 128 roundings of two such sums, is kept as the assertion);
* gradients: test_gpu_update_parity's bar (1e-5 of max|g| against the fp64 oracle evaluated at the GPU
  forward's ReLU patterns), two runs bit-equal; the distance to the unfused gradients is printed, and since
  the weight-gradient launches are the unfused ones on bit-equal inputs it is also asserted to be zero;
* the range flag, and that bytes past the data are never read;
* which shapes take the fused launch (counted through the binding), and MARLMAZE_CRITIC_FUSED=0.

Sizes: the row threshold itself (16,384), a ragged tail in the 16-row tile (+37), and 70,001 rows (more
16-row tiles than waves in the grid: every wave loops).
Reference: PPO.py:78-80, networks.py:96-102.
"""
import collections
import copy

import pytest
import torch

from marlmaze import _lib, networks, update, x3
from marlmaze.networks import Critic
from oracle import ppo as oppo

pytestmark = pytest.mark.gpu

SIZES = [16384, 16384 + 37, 70001]


@pytest.fixture(scope="module")
def nets(golden):
    fx = golden("nets")
    oc = oppo.OCritic()
    oc.load_state_dict({k[7:]: torch.as_tensor(fx[k]) for k in fx.files if k.startswith("critic/")})
    return fx, oc


def _critic(oc, prec="x2", hidden=(64, 64)):
    c = Critic(2, hidden_sizes=list(hidden), gemm_prec=prec).cuda()
    if tuple(hidden) == (64, 64):
        c.load_state_dict({k: v.detach().cuda() for k, v in oc.state_dict().items()})
    return c


def _rows(fx, M):
    """The fixture's observations tiled with noise (as test_gpu_update_parity._minibatch(fx, M, noise=0.05))."""
    g = torch.Generator().manual_seed(M)
    obs = torch.as_tensor(fx["obs"])
    obs = obs[torch.arange(M) % obs.shape[0]]
    obs = obs + 0.05 * torch.randn(obs.shape, generator=g)
    return obs.reshape(M, -1).cuda(), torch.randn(M, generator=g).cuda()


def _loss(part, M):
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    update.losses_final(torch.zeros(1, device="cuda"), part, M, out)
    return float(out[1])


def _unfused(c, x, rtg):
    """Today's launches: (V, loss, the six gradients, the saved activations)."""
    with x3.cached_packs():
        V, saved = c.train_forward(x)
        part, dv = update.mse_loss(V, rtg)
        with x3.deferred():
            c.train_backward(saved, dv)
    return V, _loss(part, x.shape[0]), [p.grad.detach().clone() for p in c._params()], saved


def _fused(c, x, rtg):
    with x3.cached_packs():
        V, part = c.train_update_fused(x, rtg)
    return V, _loss(part, x.shape[0]), [p.grad.detach().clone() for p in c._params()]


_CASES = {}


def _case(nets, M):
    """Per size, computed once: the inputs, the unfused results and the fp64 oracle at the GPU's patterns."""
    if M not in _CASES:
        fx, oc = nets
        x, rtg = _rows(fx, M)
        c = _critic(oc)
        V, loss, grads, (hs, _) = _unfused(c, x, rtg)
        pats = [(h > 0).cpu() for h in hs[1:]]
        oc64 = copy.deepcopy(oc).double()
        l64 = torch.nn.MSELoss()(oc64(x.cpu().double(), pats).squeeze(), rtg.cpu().double())
        g64 = torch.autograd.grad(l64, list(oc64.parameters()))
        names = [k for k, _ in oc64.named_parameters()]
        _CASES[M] = dict(x=x, rtg=rtg, c=c, V=V, loss=loss, grads=grads, names=names,
                         g64=dict(zip(names, g64)), l64=float(l64.detach()))
    return _CASES[M]


@pytest.mark.parametrize("M", SIZES)
def test_forward_bits_and_loss(nets, M):
    k = _case(nets, M)
    assert k["c"].fused_update_ok(k["x"])
    V, loss, _ = _fused(k["c"], k["x"], k["rtg"])
    assert V.shape == k["V"].shape and torch.equal(V, k["V"])
    print(f"M {M}: loss fused {loss!r} unfused {k['loss']!r} fp64 {k['l64']!r}")
    assert abs(loss - k["loss"]) <= 128 * 2.0 ** -24 * abs(k["loss"])


@pytest.mark.parametrize("M", SIZES)
def test_gradients_meet_the_parity_bar_and_repeat(nets, M):
    from test_gpu_update_parity import _check_grads

    k = _case(nets, M)
    _, _, g1 = _fused(k["c"], k["x"], k["rtg"])
    _, _, g2 = _fused(k["c"], k["x"], k["rtg"])
    for n, a, b, u in zip(k["names"], g1, g2, k["grads"]):
        assert torch.equal(a, b), n  # deterministic
        r = k["g64"][n]
        print(f"M {M} {n}: fused vs unfused {(a - u).abs().max().item() / r.abs().max().item():.2e} of max|g|, "
              f"fused vs fp64 {(a.cpu().double() - r).abs().max().item() / r.abs().max().item():.2e}, "
              f"unfused vs fp64 {(u.cpu().double() - r).abs().max().item() / r.abs().max().item():.2e}")
    _check_grads({n: g.cpu() for n, g in zip(k["names"], g1)}, k["g64"], f"fused critic M={M}")
    for n, a, u in zip(k["names"], g1, k["grads"]):
        assert torch.equal(a, u), n  # the same reductions on bit-equal inputs


def test_range_flag(nets):
    M = SIZES[1]
    k = _case(nets, M)
    c, x, rtg = k["c"], k["x"], k["rtg"]
    x3.range_flag(clear=True)
    V, _, g = _fused(c, x, rtg)
    assert int(x3.range_flag(clear=True).item()) == 0  # in range: clear
    # the returns x 2^20 (test_gpu_dp_range's construction): dV times the gradient scale leaves fp16's range
    _fused(c, x, rtg * 2.0 ** 20)
    assert int(x3.range_flag(clear=True).item()) != 0
    # NaN bytes after the last row and after each row's K0 columns (rows of pitch 132): never read
    K0 = x.shape[1]
    big = torch.full(((M + 64) * (K0 + 2),), float("nan"), device="cuda")
    xs = big[:M * (K0 + 2)].view(M, K0 + 2)[:, :K0]
    xs.copy_(x)
    rbig = torch.full((M + 64,), float("nan"), device="cuda")
    rbig[:M] = rtg
    assert c.fused_update_ok(xs) and xs.stride(0) == K0 + 2
    V2, _, g2 = _fused(c, xs, rbig[:M])
    assert int(x3.range_flag(clear=True).item()) == 0
    assert torch.equal(V2, V) and all(torch.equal(a, b) for a, b in zip(g, g2))


class _Counting:
    """The loaded library with every call counted by export name."""

    def __init__(self, L):
        self._L, self.calls = L, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._L, name)

        def call(*a):
            self.calls[name] += 1
            if name == "mm_mse_loss" and a[3] is not None:  # the separate launches' form: dV wanted
                self.calls["mm_mse_loss with dv"] += 1
            return f(*a)

        return call


def test_eligibility_by_counted_calls(nets, monkeypatch):
    from test_gpu_update_parity import _agent, _minibatch, _oracle_nets, _to_gpu

    fx, oc = nets
    ag = _agent(n_envs=64)
    _to_gpu(ag, *_oracle_nets(fx))
    cnt = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: cnt)

    def run(S, fused_calls):
        cnt.calls.clear()
        ag.minibatch_grads(*(t.cuda() for t in _minibatch(fx, S, noise=0.05)))
        torch.cuda.synchronize()
        assert cnt.calls["mm_critic_update"] == fused_calls, (S, dict(cnt.calls))
        assert cnt.calls["mm_mse_loss with dv"] == 1 - fused_calls, (S, dict(cnt.calls))

    assert ag.gemm_prec == "x2"
    run(16384, 1)
    run(16384 - 1, 0)  # below the B-resident kernel's row threshold
    ag.set_gemm_prec("x3")
    run(16384, 0)
    ag.set_gemm_prec("x2")
    ag.critic = _critic(oc, hidden=(32, 32))  # other widths
    run(16384, 0)
    ag.critic = _critic(oc)
    monkeypatch.setattr(networks, "CRITIC_FUSED", False)  # MARLMAZE_CRITIC_FUSED=0
    run(16384, 0)


def test_switch_off_gives_the_separate_launches_bit_for_bit(nets, monkeypatch):
    """MARLMAZE_CRITIC_FUSED=0 (networks.CRITIC_FUSED False): PPO.minibatch_grads' critic is the separate
    launches again -- its loss and gradients equal the explicit train_forward / mse_loss / train_backward
    sequence bit for bit."""
    from test_gpu_update_parity import _agent, _minibatch, _oracle_nets, _to_gpu

    fx, _ = nets
    S = SIZES[0]
    ag = _agent(n_envs=64)
    _to_gpu(ag, *_oracle_nets(fx))
    batch = [t.cuda() for t in _minibatch(fx, S, noise=0.05)]
    monkeypatch.setattr(networks, "CRITIC_FUSED", False)
    assert not ag.critic.fused_update_ok(batch[0].reshape(S, -1))
    _, cl = ag.minibatch_grads(*batch)
    cl = float(cl)
    got = [p.grad.detach().clone() for p in ag.critic._params()]
    _, loss, ref, _ = _unfused(ag.critic, batch[0].reshape(S, -1), batch[4])
    assert cl == loss
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
