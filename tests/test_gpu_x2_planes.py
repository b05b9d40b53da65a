"""x2 plane storage of the update's hidden activations and input gradients (networks.X2_PLANES, x3.planes):
fp16 [M, width / 4, 2, 4], per row and group of four columns the hi halves then the lo halves of the split every
x2 kernel applies to an fp32 operand anyway (hi = fp16(x s), lo = fp16(2^11 (x s - hi))).  The MFMA operands and
their order are those of fp32 storage, so every plane form must equal its fp32-storage form in the same build BIT FOR BIT
(test_gpu_f16_act.py's method): the producers write pair2 of what they would have stored, the GEMMs and the
weight-gradient kernel (k_wgrad_tr against k_wgrad_dma) give the same outputs from either storage, and the
update built on them gives the same gradients, parameters and logits.

Inputs are drawn like the existing tests' (activations relu(randn), gradients randn / M): no pre-scaled
gradient is subnormal in fp32, the one case where pair2(x s) and the scaled pair2(x) could differ.
The front-end output h0 stays fp32 (so do dY1, the 264 x 460 weight gradient's operands and the 460-wide
input gradient's A): plane storage covers h1, h2, dY3, dY2, and the library has the plane forms of the hidden
layers only -- a plane A goes through ReLU bits, and the plane weight gradient has the 264 x 264 blocks.
"""
import pytest
import torch

from marlmaze import _lib, networks, x3

pytestmark = pytest.mark.gpu

MS = [1, 17, 255, 257, 3001, 16384 + 33]  # the last: just above the B-resident kernel's row threshold
SHAPES = [(264, 264), (264, 460)]


def to_planes(x, s=1.0, pad=None):
    """pair2 in torch: the plane tensor of x s.  pad: the tensor is the leading columns of one 16 columns
    wider (a row pitch, as a strided fp32 matrix has), whose other columns hold ``pad`` in both planes."""
    M, n = x.shape
    v = x * s
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    if pad is None:
        p = x3.planes(M, n, x.device)
    else:
        p = torch.full((M, n // 4 + 4, 2, 4), pad, dtype=torch.float16, device=x.device)[:, :n // 4]
    p[:, :, 0, :] = hi.view(M, n // 4, 4)
    p[:, :, 1, :] = lo.view(M, n // 4, 4)
    return p


def planes_equal(p, x, s=1.0):
    return torch.equal(p.view(torch.int16), to_planes(x, s).view(torch.int16))


def _bits_of(M, N, g):
    """ReLU bits of some [M, N] forward (zeroed first: the kernels leave the words' padding bits unwritten)."""
    mb = x3.mbits(M, "cuda").zero_()
    x3.gemm(torch.randn(M, 64, device="cuda", generator=g),
            x3.pack(torch.randn(N, 64, device="cuda", generator=g), prec="x2"), relu=True, mbits_out=mb)
    return mb


# ---- producers ----

@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_forward_writes_the_planes_of_its_fp32_output(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + K)
    a = torch.relu(torch.randn(M, K, device="cuda", generator=g))
    w = x3.pack(torch.randn(N, K, device="cuda", generator=g) * 0.1, prec="x2")
    b = torch.randn(N, device="cuda", generator=g)
    mbp, mb32 = x3.mbits(M, "cuda").zero_(), x3.mbits(M, "cuda").zero_()
    y32 = x3.gemm(a, w, bias=b, relu=True, mbits_out=mb32)
    yp = x3.gemm(a, w, bias=b, relu=True, mbits_out=mbp, out=x3.planes(M, N, "cuda"))
    assert x3.is_planes(yp) and planes_equal(yp, y32)
    assert torch.equal(mbp, mb32)  # the bits come from the fp32 value


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_input_gradient_writes_the_prescaled_planes(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + 5 * N + K)
    s = networks._grad_scale(M, "x2")
    dy = torch.randn(M, K, device="cuda", generator=g) / M
    w = x3.pack(torch.randn(K, N, device="cuda", generator=g) * 0.1, trans=True, prec="x2")  # W [K, N]^T
    mb = _bits_of(M, N, g)
    cs32, csp = x3.colsum_buf(M, N, "cuda"), x3.colsum_buf(M, N, "cuda")
    o32 = x3.gemm(dy, w, mbits_in=mb, colsum=cs32, ascale=s)
    op = x3.gemm(dy, w, mbits_in=mb, colsum=csp, ascale=s, out=x3.planes(M, N, "cuda"), oscale=s)
    assert planes_equal(op, o32, s)
    assert torch.equal(csp, cs32)  # the column sums stay those of the fp32 values


@pytest.mark.parametrize("M", MS)
def test_heads_bwd_writes_the_prescaled_planes(M):
    g = torch.Generator(device="cuda").manual_seed(13 + M)
    s = networks._grad_scale(M, "x2")
    dz = torch.randn(M, 6, device="cuda", generator=g) / M
    w = torch.randn(6, 264, device="cuda", generator=g) * 0.1
    mb = _bits_of(M, 264, g)
    dy32, cs32 = x3.heads_bwd(dz, w, mb)
    dyp, csp = x3.heads_bwd(dz, w, mb, oscale=s, x2p=True)
    assert x3.is_planes(dyp) and planes_equal(dyp, dy32, s) and torch.equal(csp, cs32)


# ---- GEMM consumers ----

@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_forward_from_planes_equals_forward_from_fp32(M, N, K):
    """K = 460 runs on the streaming kernel (its two-plane A source) at every M, K = 264 on the B-resident
    kernel from its row threshold; fp32 and plane outputs."""
    g = torch.Generator(device="cuda").manual_seed(M + 7 * N + K)
    a = torch.relu(torch.randn(M, K, device="cuda", generator=g))
    ap = to_planes(a, pad=float("nan"))  # (a row pitch past K; the columns past K are never read)
    w = x3.pack(torch.randn(N, K, device="cuda", generator=g) * 0.1, prec="x2")
    b = torch.randn(N, device="cuda", generator=g)
    mbp, mb32 = x3.mbits(M, "cuda").zero_(), x3.mbits(M, "cuda").zero_()
    y32 = x3.gemm(a, w, bias=b, relu=True, mbits_out=mb32)
    yp = x3.gemm(ap, w, bias=b, relu=True, mbits_out=mbp)
    assert yp.dtype == torch.float32 and torch.equal(yp, y32) and torch.equal(mbp, mb32)
    ypp = x3.gemm(ap, w, bias=b, relu=True, mbits_out=mbp, out=x3.planes(M, N, "cuda"))
    assert planes_equal(ypp, y32)


@pytest.mark.parametrize("M", MS)
def test_input_gradient_from_planes_equals_input_gradient_from_fp32(M, N=264, K=264):
    """gemm(planes of dY s, W^T) at ascale 1, cscale 1 / s == gemm(dY, W^T) at ascale s, through the ReLU bits
    into planes again or into fp32 (the gradient into a layer whose input is stored fp32)."""
    g = torch.Generator(device="cuda").manual_seed(M + 11 * N + K)
    s = networks._grad_scale(M, "x2")
    dy = torch.randn(M, K, device="cuda", generator=g) / M
    dyp = to_planes(dy, s, pad=float("nan"))
    w = x3.pack(torch.randn(K, N, device="cuda", generator=g) * 0.1, trans=True, prec="x2")
    mb = _bits_of(M, N, g)
    cs32, csp = x3.colsum_buf(M, N, "cuda"), x3.colsum_buf(M, N, "cuda")
    o32 = x3.gemm(dy, w, mbits_in=mb, colsum=cs32, ascale=s)
    op = x3.gemm(dyp, w, mbits_in=mb, colsum=csp, ascale=1.0, cscale=1.0 / s, out=x3.planes(M, N, "cuda"),
                 oscale=s)
    assert planes_equal(op, o32, s) and torch.equal(csp, cs32)
    o = x3.gemm(dyp, w, mbits_in=mb, colsum=csp, ascale=1.0, cscale=1.0 / s)  # fp32 out (into an fp32 layer)
    assert o.dtype == torch.float32 and torch.equal(o, o32)


def test_plane_forms_outside_the_hidden_layers_are_refused():
    """No plane A without ReLU bits (the 460-wide gradient into the front end reads fp32 dY1) and no plane
    weight gradient at 264 x 460 (h0 is fp32): an error, never another kernel."""
    M = 64
    dyp = to_planes(torch.randn(M, 264, device="cuda") / M, 64.0)
    w = x3.pack(torch.randn(264, 460, device="cuda") * 0.1, trans=True, prec="x2")
    with pytest.raises(_lib.MMError):
        x3.gemm(dyp, w, ascale=1.0, cscale=1.0 / 64.0)
    assert not x3.x2p_ok(M, 264, 460)
    with pytest.raises(_lib.MMError):
        x3.wgrad(dyp, to_planes(torch.randn(M, 460, device="cuda")), prec="x2", dscale=1.0, cscale=1.0 / 64.0,
                 nk=(264, 460))


# ---- the weight gradient: k_wgrad_tr (planes) against k_wgrad_dma (fp32) ----

def _wgrad_pair(M, N, K, seed, pad=None, poke=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = networks._grad_scale(M, "x2")
    dy = torch.randn(M, N, device="cuda", generator=g) / M
    x = torch.relu(torch.randn(M, K, device="cuda", generator=g))
    if poke is not None:
        x[min(5, M - 1), 7] = poke
    return s, dy, x, to_planes(dy, s, pad), to_planes(x, 1.0, pad)


def _partials(M, N, K, dy, x, s, planes):
    L = _lib.lib()
    S = L.mm_gemm_wgrad_slices(_lib.PREC_X2, M, N, K)
    assert S > 0
    ws = torch.full((S, N, K), float("nan"), dtype=torch.float32, device="cuda")
    if planes:
        rc = L.mm_gemm_wgrad_partials_h(_lib.PREC_X2, _lib.GEMM_A_X2P | _lib.GEMM_B_X2P, _lib.ptr(dy),
                                        dy.stride(0) // 2, 1.0, _lib.ptr(x), x.stride(0) // 2, M, N, K, 1.0 / s,
                                        _lib.ptr(ws), _lib.stream_ptr())
    else:
        rc = L.mm_gemm_wgrad_partials(_lib.PREC_X2, _lib.ptr(dy), dy.stride(0), s, _lib.ptr(x), x.stride(0), M, N, K,
                                      1.0 / s, _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "mm_gemm_wgrad_partials")
    return S, ws


# 1 to 5 steps of 32 rows and a ragged last step (every fill state of the three-stage ring); 20,011: several
# slices on any grid, the last one ragged
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 96, 97, 160, 1000, 20011])
def test_wgrad_planes_equals_wgrad_dma(M, N=264, K=264):
    assert x3.x2p_ok(M, N, K)
    s, dy, x, dyp, xp = _wgrad_pair(M, N, K, M + N + K)
    prev = x3.set_wgrad_algo("dma")
    try:
        S, p32 = _partials(M, N, K, dy, x, s, False)
        Sp, pp = _partials(M, N, K, dyp, xp, s, True)
        # (slices are whole 32-row steps, so with M % 32 != 0 the last slice is ragged)
        assert S == Sp and (M < 20000 or S >= 2)
        assert torch.equal(pp, p32)
        d32 = x3.wgrad(dy, x, prec="x2", dscale=s)
        dp = x3.wgrad(dyp, xp, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert torch.equal(dp, d32)
    finally:
        x3.set_wgrad_algo(prev)


def test_wgrad_planes_ignores_nan_padding():
    """The columns between an operand's width and its row pitch -- which the tile columns past N / K read --
    hold fp16 NaNs in both planes: the result is unchanged and the range flag stays clear (only stored
    accumulators are range-checked)."""
    M, N, K = 1000, 260, 260  # 17 x 16 = 272 > 260 and 2 x 9 x 16 = 288 > 260: tile columns in the NaNs
    assert x3.x2p_ok(M, N, K)
    s, dy, x, dyp, xp = _wgrad_pair(M, N, K, 77, pad=float("nan"))
    assert not dyp.is_contiguous() and dyp.stride(0) == 2 * (N + 16) and xp.stride(0) == 2 * (K + 16)
    prev = x3.set_wgrad_algo("dma")
    try:
        d32 = x3.wgrad(dy, x, prec="x2", dscale=s)
        x3.range_flag(clear=True)
        dp = x3.wgrad(dyp, xp, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert int(x3.range_flag(clear=True).item()) == 0
        assert torch.equal(dp, d32)
    finally:
        x3.set_wgrad_algo(prev)


def test_wgrad_planes_raises_the_range_flag():
    """One in-range operand at 7e4 (past fp16): its hi plane is inf, and the flag is set as k_wgrad_dma sets it."""
    M, N, K = 160, 264, 264
    s, dy, x, dyp, xp = _wgrad_pair(M, N, K, 78, poke=7e4)
    prev = x3.set_wgrad_algo("dma")
    try:
        x3.range_flag(clear=True)
        x3.wgrad(dy, x, prec="x2", dscale=s)
        assert int(x3.range_flag(clear=True).item()) != 0
        x3.wgrad(dyp, xp, prec="x2", dscale=1.0, cscale=1.0 / s, nk=(N, K))
        assert int(x3.range_flag(clear=True).item()) != 0
    finally:
        x3.set_wgrad_algo(prev)


# ---- end to end ----

@pytest.mark.parametrize("S", [3000, 6001])
def test_update_with_planes_is_bit_identical(golden, monkeypatch, S):
    """PPO.minibatch_grads + minibatch_step with plane storage on and off: the flat gradient buffer, the
    parameters after the step and train_forward's logits are equal bit for bit -- and the plane path ran."""
    from test_gpu_update_parity import _agent, _minibatch, _oracle_nets, _to_gpu

    fx = golden("nets")
    batch = [t.cuda() for t in _minibatch(fx, S, noise=0.05)]
    res = []
    for on in (False, True):
        monkeypatch.setattr(networks, "X2_PLANES", on)
        actor, critic = _oracle_nets(fx)
        ag = _agent(n_envs=64)
        assert ag.gemm_prec == "x2"
        _to_gpu(ag, actor, critic)
        z, saved = ag.actor.train_forward(batch[0].reshape(2 * S, 65))
        hs = saved[2]
        assert hs[0].dtype == torch.float32 and hs[3].dtype == torch.float32
        for h in hs[1:3]:  # stored as fp16 planes; to torch the fp32 [M, 264] matrix either way
            assert isinstance(h, networks._SavedPlanes) == on
            assert h.shape == (2 * S, 264) and h.dtype == torch.float32 and (h > 0).shape == h.shape
            assert (on and h.planes().dtype == torch.float16 and x3.is_planes(h.planes())) == on
        ag.minibatch_grads(*batch)
        grads = ag.flat.grad.clone()
        out = ag.minibatch_step(*batch)
        torch.cuda.synchronize()
        res.append((z.clone(), grads, torch.stack(out).cpu(), ag.flat.data.clone(), ag.flat.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
