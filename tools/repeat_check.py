"""Run-to-run determinism check of single GEMM calls across library builds (in one process): each case is
run REPS times per library; prints the error against fp64 and whether every repeat was bitwise identical.

  LIBS=tools/_var/base.so,marl-maze_amd/libmarlmaze.so python tools/repeat_check.py

With two LIBS it then compares the builds bit for bit (SWEEP=0 skips this): every GEMM form at the smallest
shapes that reach each code path of the streaming and the B-resident kernel -- the status each library returns
and, where the first library accepts the call, every output of its first launch -- and the row-chunk path,
mm_x3_nt, the fused trunk, mm_critic_update and the heads' backward.  Prints one line per case that differs and
the totals; exit status 1 when any case differs.
"""
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "marl-maze_amd"))
import torch  # noqa: E402

from marlmaze import _lib, x3  # noqa: E402


def load(path):
    _lib.LIB_PATH = path
    _lib._LIB = None
    return _lib.lib()


def rel(a, ref, scale):
    return ((a.double() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def cases():
    g = torch.Generator(device="cuda").manual_seed(40270)
    M, N, K = 40000, 6, 264
    dy = torch.randn(M, N, device="cuda", generator=g) / M
    x = torch.randn(M, K, device="cuda", generator=g)
    s = float(2 ** 15)
    ref = dy.double().t().mm(x.double())
    sc = dy.double().abs().t().mm(x.double().abs())
    yield "wgrad x2 40000x6x264", (lambda: x3.wgrad(dy, x, prec="x2", dscale=s)), ref, sc
    for prec, M, N, K in (("x2", 419430, 264, 264), ("x2", 209715, 64, 130), ("f16", 100000, 264, 264)):
        a = torch.randn(M, K, device="cuda", generator=g)
        w = torch.randn(N, K, device="cuda", generator=g) * 0.05
        b = torch.randn(N, device="cuda", generator=g)
        ref2 = (a.double() @ w.double().t() + b.double()).clamp_min(0)
        sc2 = a.double().abs() @ w.double().abs().t() + b.double().abs()
        yield (f"gemm {prec} fwd {M}x{N}x{K}",
               (lambda a=a, w=w, b=b, p=prec: x3.gemm(a, x3.pack(w, prec=p), bias=b, relu=True)), ref2, sc2)
    from marlmaze.networks import _heads_fwd
    h = torch.randn(419430, 264, device="cuda", generator=g).clamp_min(0)
    wh = torch.randn(6, 264, device="cuda", generator=g) * 0.01
    bh = torch.randn(6, device="cuda", generator=g)
    yield "heads_fwd 419430x264", (lambda: _heads_fwd(h, wh, bh)), h.double() @ wh.double().t() + bh.double(), \
        h.double().abs() @ wh.double().abs().t() + bh.double().abs()
    for prec in ("f16", "x2"):
        M, N, K = 40000, 460, 264
        a = torch.randn(M, K, device="cuda", generator=g)
        w = torch.randn(N, K, device="cuda", generator=g) * 0.05
        ref2 = a.double() @ w.double().t()
        sc2 = a.double().abs() @ w.double().abs().t()
        yield f"gemm {prec} plain 40000x460x264", (lambda a=a, w=w, p=prec: x3.gemm(a, x3.pack(w, prec=p))), ref2, sc2


# ---- the cross-library sweep ----

STREAM_M, STREAM_M_X2 = (1, 33, 257), (1, 33, 129, 257)  # x2's workgroups are 8 waves: 129 too
STREAM_NK = ((264, 460), (264, 264), (460, 264), (64, 130), (6, 264), (1, 64))
BRES_M = (16384, 16417)  # the row threshold, and a ragged last tile
BRES_NK = ((264, 264), (460, 264), (64, 130), (6, 264))
A_FORMS = ("f32", "f32u", "f16", "x2p")  # fp32 16-byte rows, fp32 8-byte rows, fp16 rows, x2 planes
C_FORMS = ("f32", "f16", "x2p")
FORMS = ("fwd", "bwd", "plain")  # forward with bits; input gradient with bits and column sums; no bits


def to_planes(x):
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    M, n = x.shape
    return torch.stack((hi.view(M, n // 4, 4), lo.view(M, n // 4, 4)), dim=2).contiguous()


class Shape:
    """The operands of one (M, N, K), made once and shared by its cases and both libraries."""

    def __init__(self, M, N, K, g):
        self.M, self.N, self.K = M, N, K
        self.a = torch.randn(M, K, device="cuda", generator=g)
        flat = torch.zeros(M * K + 4, device="cuda")  # the same values 8 bytes off a 16-byte boundary
        flat[2:2 + M * K] = self.a.reshape(-1)
        self.a_u = flat[2:2 + M * K].view(M, K)
        self.a16 = self.a.half()
        self.ap = to_planes(self.a) if K % 4 == 0 else None
        self.w = torch.randn(N, K, device="cuda", generator=g) * 0.05
        self.bias = torch.randn(N, device="cuda", generator=g)
        self.bits = None

    def bits_in(self):
        if self.bits is None:  # a forward's mask of the [M, N] tiling (N > 272: no mask; the calls are refused)
            self.bits = x3.mbits(self.M, "cuda").zero_()
            if self.N <= 272:
                x3.gemm(self.a, x3.pack(self.w, prec="x3"), relu=True, mbits_out=self.bits)
        return self.bits


def gemm_call(L, sh, prec, form, af, cf):
    """One mm_gemm_nt_h call: (status, outputs)."""
    M, N, K = sh.M, sh.N, sh.K
    if (af == "x2p" and sh.ap is None) or (cf == "x2p" and N % 4):
        return None
    a = {"f32": sh.a, "f32u": sh.a_u, "f16": sh.a16, "x2p": sh.ap}[af]
    flags = {"f32": 0, "f32u": 0, "f16": _lib.GEMM_A_F16, "x2p": _lib.GEMM_A_X2P}[af]
    flags |= {"f32": 0, "f16": _lib.GEMM_C_F16, "x2p": _lib.GEMM_C_X2P}[cf]
    out = (torch.zeros((M, N), dtype=torch.float16, device="cuda") if cf == "f16"
           else x3.planes(M, N, "cuda").zero_() if cf == "x2p" else torch.zeros(M, N, device="cuda"))
    stored = af in ("f16", "x2p")  # read at scale 1
    ascale = 1.0 if (prec == "x3" or stored) else 4.0
    cscale = 1.0 if prec == "x3" else 0.25
    mb_out = x3.mbits(M, "cuda").zero_() if form == "fwd" else None
    cs = x3.colsum_buf(M, N, "cuda").zero_() if form == "bwd" else None
    wp = x3.pack(sh.w, prec=prec)
    rc = L.mm_gemm_nt_h(x3.PRECS[prec], flags, _lib.ptr(a), K, ascale, wp.ptr(), M, N, K,
                        _lib.ptr(sh.bias) if form != "bwd" else None, int(form == "fwd"),
                        _lib.ptr(sh.bits_in()) if form == "bwd" else None, _lib.ptr(mb_out), _lib.ptr(cs), cscale,
                        4.0 if form == "bwd" and cf != "f32" else 1.0, _lib.ptr(out), N, _lib.stream_ptr())
    return rc, [t for t in (out, mb_out, cs) if t is not None]


def sweep_cases(g):
    """(name, fn): fn(L) -> (status, [output tensors]) or None (the form does not exist at the shape)."""
    for Ms, NKs, fam in ((None, STREAM_NK, "stream"), (BRES_M, BRES_NK, "bres")):
        for N, K in NKs:
            for M in (Ms or STREAM_M_X2):
                sh = Shape(M, N, K, g)
                for prec, form, af, cf in itertools.product(("x3", "x2", "f16"), FORMS, A_FORMS, C_FORMS):
                    if fam == "stream" and M == 129 and prec != "x2":
                        continue
                    yield (f"{fam} {prec} {form} A {af} C {cf} {M}x{N}x{K}",
                           lambda L, sh=sh, p=prec, f=form, a=af, c=cf: gemm_call(L, sh, p, f, a, c))
    # the row-chunk path (tests/test_gpu_gemm.py::test_gemm_row_chunks's shape): forward with bits, then the
    # input gradient through them
    M, N, K = 1_200_000, 264, 460
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.randn(N, device="cuda", generator=g)
    dy = torch.randn(M, 48, device="cuda", generator=g)
    w2 = torch.randn(48, N, device="cuda", generator=g) * 0.1

    def chunks(L):
        bits = x3.mbits(M, "cuda").zero_()
        y = x3.gemm(a, x3.pack(w), bias=b, relu=True, mbits_out=bits)
        cs = x3.colsum_buf(M, N, "cuda").zero_()
        dx = x3.gemm(dy, x3.pack(w2, trans=True), mbits_in=bits, colsum=cs)
        return 0, [y, bits, dx, cs]
    yield "row chunks 1200000x264x460", chunks
    del chunks
    # mm_x3_nt: TP A, TP C, the fp32 mask
    for M in (33, 257):
        a3 = torch.randn(M, 264, device="cuda", generator=g)
        w3 = torch.randn(264, 264, device="cuda", generator=g) * 0.05
        mk = torch.randn(M, 264, device="cuda", generator=g)

        def nt(L, a3=a3, w3=w3, mk=mk, M=M):
            atp, wtp = x3.pack(a3), x3.pack(w3)
            c1, _ = x3.nt(atp, wtp, bias=b, relu=True, mask=mk)
            ctp = x3.TP(M, 264, "cuda")
            ctp.buf.zero_()
            x3.nt(atp, wtp, bias=b, relu=True, out_tp=ctp, want_f32=False)
            c2, _ = x3.nt(a3, wtp, mask=mk)
            ctp2 = x3.TP(M, 264, "cuda")
            ctp2.buf.zero_()
            x3.nt(a3, wtp, bias=b, out_tp=ctp2, want_f32=False)
            return 0, [c1, ctp.buf, c2, ctp2.buf]
        yield f"mm_x3_nt TP A / TP C / mask {M}", nt
    # the fused trunk and trunk + heads + sampler
    hw, hb = torch.randn(6, 264, device="cuda", generator=g) * 0.2, torch.randn(6, device="cuda", generator=g) * 0.1
    ws = [torch.randn(264, k, device="cuda", generator=g) * 0.05 for k in (460, 264, 264)]
    bs = [torch.randn(264, device="cuda", generator=g) * 0.1 for _ in range(3)]
    for M in (1, 33, 8195):
        h0 = torch.relu(torch.randn(M, 460, device="cuda", generator=g))
        mk6 = (torch.rand(M, 6, device="cuda", generator=g) < 0.6).to(torch.uint8)
        mk6[:, 4] = 1
        for prec in ("x3", "x2", "f16"):
            def trunk(L, h0=h0, prec=prec):
                return 0, [x3.trunk3(h0, [x3.pack(w_, prec=prec) for w_ in ws], bs)]

            def trunk_hs(L, h0=h0, mk6=mk6, prec=prec, M=M):
                o = [torch.zeros((M, 2), dtype=torch.int8, device="cuda"), torch.zeros(M, device="cuda"),
                     torch.zeros((M + 1) // 2, device="cuda"), torch.zeros(M, 6, device="cuda"),
                     torch.zeros(M, 264, device="cuda")]
                x3.trunk3_head_sample(h0, [x3.pack(w_, prec=prec) for w_ in ws], bs, hw, hb, mk6, 4321, 9, o[0], o[1],
                                      o[2], logits=o[3], h3=o[4])
                return 0, o
            yield f"mm_trunk3 {prec} {M}", trunk
            yield f"mm_trunk3_head_sample {prec} {M}", trunk_hs
    # mm_critic_update (tests/test_gpu_critic_fused.py's SIZES)
    from marlmaze.networks import Critic
    torch.manual_seed(5)
    critic = Critic(2, hidden_sizes=[64, 64], gemm_prec="x2").cuda()
    for M in (16384, 16384 + 37, 70001):
        xc = torch.randn(M, 130, device="cuda", generator=g)
        rtg = torch.randn(M, device="cuda", generator=g)

        def cu(L, xc=xc, rtg=rtg):
            x3.invalidate_packs()
            with x3.cached_packs():
                V, part = critic.train_update_fused(xc, rtg)
            return 0, [V, part] + [p.grad.detach().clone() for p in critic._params()]
        yield f"mm_critic_update {M}", cu
    # the heads' backward: fp32, fp16 and plane dY
    wh = torch.randn(6, 264, device="cuda", generator=g) * 0.1
    for M in (1, 33):
        sh = Shape(M, 264, 64, g)
        dz = torch.randn(M, 6, device="cuda", generator=g)
        for kw in (dict(), dict(oscale=4.0), dict(oscale=4.0, x2p=True)):
            yield f"mm_x3_heads_bwd {kw} {M}", (lambda L, sh=sh, dz=dz, kw=kw: (0, list(x3.heads_bwd(dz, wh, sh.bits_in(), **kw))))


def sweep(libs, Ls):
    g = torch.Generator(device="cuda").manual_seed(777)
    ran = accepted = differ = 0
    for name, fn in sweep_cases(g):
        res = []
        for L in Ls:
            _lib._LIB = L
            res.append(fn(L))
        torch.cuda.synchronize()
        if res[0] is None:
            continue
        ran += 1
        (rc0, out0), (rc1, out1) = res
        same = rc0 == rc1 and (rc0 != 0 or all(
            torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in zip(out0, out1)))
        accepted += int(rc0 == 0)
        if not same:
            differ += 1
            print(f"DIFFERS {name}: status {rc0} / {rc1}", flush=True)
    print(f"sweep {os.path.basename(libs[0])} vs {os.path.basename(libs[1])}: {ran} cases, {accepted} accepted by the "
          f"first library and compared bit for bit, {differ} differ", flush=True)
    return differ


def main():
    libs = os.environ.get("LIBS", "tools/_var/base.so,marl-maze_amd/libmarlmaze.so").split(",")
    reps = int(os.environ.get("REPS", 30))
    Ls = []
    for path in libs:
        Ls.append(load(os.path.join(REPO, path) if not os.path.isabs(path) else path))
        for name, fn, ref, sc in cases():
            outs = [fn().clone() for _ in range(reps)]
            torch.cuda.synchronize()
            same = all(torch.equal(outs[0], o) for o in outs[1:])
            errs = [rel(o, ref, sc) for o in outs]
            print(f"{os.path.basename(path):16s} {name:28s} max err {max(errs):.3e} min err {min(errs):.3e} "
                  f"identical repeats {same}", flush=True)
    if len(Ls) == 2 and os.environ.get("SWEEP", "1") != "0":
        sys.exit(1 if sweep(libs, Ls) else 0)


if __name__ == "__main__":
    main()
