"""dY1 -- the gradient into the first trunk layer -- stored as pre-scaled x2 planes beside the fp32 h0
(networks.X2_DY1): the 264 x 460 weight gradient reads the plane dY with an fp32 X (k_wgrad_mix), and the 460-wide
input gradient is a plane-A GEMM without ReLU bits on the B-resident kernel.  Both feed the MFMAs the operands
the fp32-dY forms feed them, in the same order, so everything here is compared BIT FOR BIT with the fp32 form of
the same build (test_gpu_x2_planes.py's method and helpers): the mixed kernel's row-slice partials against
k_wgrad_dma's, the plain plane-A GEMM against the fp32-A launch, and the update with the switch on and off.
"""
import pytest
import torch

from marlmaze import _lib, networks, x3
from test_gpu_x2_planes import _wgrad_pair, to_planes

pytestmark = pytest.mark.gpu

N1, K1 = 264, 460  # dW1 = dY1^T h0


def _nan_pitch(x):
    """x as the leading columns of an fp32 matrix 16 columns wider whose other columns hold NaNs."""
    M, n = x.shape
    p = torch.full((M, n + 16), float("nan"), dtype=torch.float32, device=x.device)[:, :n]
    p.copy_(x)
    return p


def _partials(M, N, K, dy, x, s, mixed):
    L = _lib.lib()
    S = L.mm_gemm_wgrad_slices(_lib.PREC_X2, M, N, K)
    assert S > 0
    ws = torch.full((S, N, K), float("nan"), dtype=torch.float32, device="cuda")
    if mixed:
        rc = L.mm_gemm_wgrad_partials_h(_lib.PREC_X2, _lib.GEMM_A_X2P, _lib.ptr(dy), dy.stride(0) // 2, 1.0,
                                        _lib.ptr(x), x.stride(0), M, N, K, 1.0 / s, _lib.ptr(ws), _lib.stream_ptr())
    else:
        rc = L.mm_gemm_wgrad_partials(_lib.PREC_X2, _lib.ptr(dy), dy.stride(0), s, _lib.ptr(x), x.stride(0), M, N, K,
                                      1.0 / s, _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "mm_gemm_wgrad_partials")
    return S, ws


# ---- the weight gradient: k_wgrad_mix (plane dY, fp32 X) against k_wgrad_dma (fp32) ----

# 1 to 5 steps of 32 rows and a ragged last step (every fill state of the two-stage ring); 20,011: several
# slices on any grid, the last one ragged
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 96, 97, 160, 1000, 20011])
def test_wgrad_mixed_equals_wgrad_dma(M, N=N1, K=K1):
    s, dy, x, dyp, _ = _wgrad_pair(M, N, K, M + N + K)
    prev = x3.set_wgrad_algo("dma")
    try:
        S, p32 = _partials(M, N, K, dy, x, s, False)
        Sm, pm = _partials(M, N, K, dyp, x, s, True)
        assert S == Sm and (M < 20000 or S >= 2)
        assert torch.equal(pm, p32)
        d32 = x3.wgrad(dy, x, prec="x2", dscale=s)
        dm = x3.wgrad(dyp, x, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert torch.equal(dm, d32)
    finally:
        x3.set_wgrad_algo(prev)


def test_wgrad_mixed_ignores_nan_padding():
    """The columns between an operand's width and its row pitch -- which the tile columns past N / K read --
    hold NaNs (fp16 NaNs in both of dY's planes, fp32 NaNs in X): the result equals the fp32 form's (on clean
    operands) and the range flag stays clear (only stored accumulators are range-checked)."""
    M, N, K = 1000, 260, 456  # 17 x 16 = 272 > 260 and 29 x 16 = 464 > 456: tile columns in the NaNs
    s, dy, x, dyp, _ = _wgrad_pair(M, N, K, 79, pad=float("nan"))
    xn = _nan_pitch(x)
    assert dyp.stride(0) == 2 * (N + 16) and xn.stride(0) == K + 16 and torch.equal(xn, x)
    prev = x3.set_wgrad_algo("dma")
    try:
        d32 = x3.wgrad(dy, x, prec="x2", dscale=s)
        x3.range_flag(clear=True)
        dm = x3.wgrad(dyp, xn, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert int(x3.range_flag(clear=True).item()) == 0
        assert torch.equal(dm, d32)
    finally:
        x3.set_wgrad_algo(prev)


def test_wgrad_mixed_raises_the_range_flag():
    """One X element at 7e4 (past fp16): its hi half is inf, and the flag is set as k_wgrad_dma sets it."""
    M, N, K = 160, N1, K1
    s, dy, x, dyp, _ = _wgrad_pair(M, N, K, 80, poke=7e4)
    prev = x3.set_wgrad_algo("dma")
    try:
        x3.range_flag(clear=True)
        x3.wgrad(dy, x, prec="x2", dscale=s)
        assert int(x3.range_flag(clear=True).item()) != 0
        x3.wgrad(dyp, x, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert int(x3.range_flag(clear=True).item()) != 0
    finally:
        x3.set_wgrad_algo(prev)


# ---- the 460-wide input gradient: a plane A without ReLU bits (the B-resident kernel) ----

def _dx_operands(M):
    g = torch.Generator(device="cuda").manual_seed(M + 17)
    s = networks._grad_scale(M, "x2")
    dy = torch.randn(M, N1, device="cuda", generator=g) / M
    wt = x3.pack(torch.randn(N1, K1, device="cuda", generator=g) * 0.1, trans=True, prec="x2")  # W1 [264, 460]^T
    return s, dy, to_planes(dy, s, pad=float("nan")), wt


@pytest.mark.parametrize("M", [16384, 16417, 20011])  # the row threshold; a ragged last row tile; several units
def test_plain_input_gradient_from_planes_equals_fp32(M):
    assert x3.x2p_dy_ok(M, N1, K1)
    s, dy, dyp, wt = _dx_operands(M)
    o32 = x3.gemm(dy, wt, ascale=s)
    op = x3.gemm(dyp, wt, ascale=1.0, cscale=1.0 / s)
    assert op.dtype == torch.float32 and op.shape == (M, K1) and torch.equal(op, o32)


def test_plain_plane_a_is_refused_off_the_b_resident_kernel():
    """Below the row threshold and under set_algo("stream") the GEMM would run on the streaming kernel, which
    takes a plane A through ReLU bits only: an error, and x2p_dy_ok says so beforehand."""
    M = 16383
    s, dy, dyp, wt = _dx_operands(M)
    assert not x3.x2p_dy_ok(M, N1, K1)
    with pytest.raises(_lib.MMError):
        x3.gemm(dyp, wt, ascale=1.0, cscale=1.0 / s)
    M = 16384
    s, dy, dyp, wt = _dx_operands(M)
    prev = x3.set_algo("stream")
    try:
        assert not x3.x2p_dy_ok(M, N1, K1)
        with pytest.raises(_lib.MMError):
            x3.gemm(dyp, wt, ascale=1.0, cscale=1.0 / s)
    finally:
        x3.set_algo(prev)
    assert x3.x2p_dy_ok(M, N1, K1)


# ---- end to end ----

@pytest.mark.parametrize("S", [8192, 8209])  # 16,384 and 16,418 actor rows: the smallest at which the path runs
def test_update_with_dy1_planes_is_bit_identical(golden, monkeypatch, S):
    """PPO.minibatch_grads + minibatch_step with X2_DY1 on and off: the flat gradient buffer, the parameters
    after the step, the step's outputs and train_forward's logits are equal bit for bit -- and the weight
    gradient saw a plane dY beside an fp32 X in the on arm only."""
    from test_gpu_update_parity import _agent, _minibatch, _oracle_nets, _to_gpu

    fx = golden("nets")
    batch = [t.cuda() for t in _minibatch(fx, S, noise=0.05)]
    real_wgrad = x3.wgrad
    res = []
    for on in (False, True):
        monkeypatch.setattr(networks, "X2_DY1", on)
        mixed = []

        def spy(dy, x, *a, **k):
            mixed.append(x3.is_planes(dy) and x.dtype == torch.float32 and not x3.is_planes(x))
            return real_wgrad(dy, x, *a, **k)

        monkeypatch.setattr(x3, "wgrad", spy)
        actor, critic = _oracle_nets(fx)
        ag = _agent(n_envs=64)
        assert ag.gemm_prec == "x2"
        _to_gpu(ag, actor, critic)
        z, saved = ag.actor.train_forward(batch[0].reshape(2 * S, 65))
        assert saved[2][0].dtype == torch.float32  # h0 stays fp32
        ag.minibatch_grads(*batch)
        grads = ag.flat.grad.clone()
        out = ag.minibatch_step(*batch)
        torch.cuda.synchronize()
        monkeypatch.setattr(x3, "wgrad", real_wgrad)
        assert mixed and any(mixed) == on
        res.append((z.clone(), grads, torch.stack(out).cpu(), ag.flat.data.clone(), ag.flat.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
