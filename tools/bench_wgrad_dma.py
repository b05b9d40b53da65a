"""x2 trunk weight gradients: k_wgrad_tr (operands stored as x2 planes, three raw stages, no conversion)
against k_wgrad_dma (fp32 operands, LDS-DMA staging, two raw stages in flight) and k_wgrad_rect (register
staging), alternating in one process, HIP events, median and min .. max of ROUNDS x 10 launches; algorithmic
bytes 4 M (N + K) per launch.  At 264 x 460 k_wgrad_mix (dY as planes beside the fp32 X) joins them.  Then the 264 x 264 forward and input-gradient GEMMs (k_bres) from plane A /
into planes against fp32 storage, the same way.  One JSON line per shape.

  python tools/bench_wgrad_dma.py [M]

MIX_LIBS=name:path[,name:path...] adds k_wgrad_mix of other builds of the library (tools/ab_build.py: e.g. a
diagnostic build with -DWG_NO_MFMA, or "base" for the parent commit's kernel) to the 264 x 460 alternation as
mix_NAME (dma_NAME for a build without the mixed kernel).
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-maze_amd"))
from marlmaze import _lib, x3  # noqa: E402

ROUNDS = 7


def timed(f, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def to_planes(x, s=1.0):
    v = x * s
    hi = v.half()
    p = x3.planes(x.shape[0], x.shape[1], x.device)
    p[:, :, 0, :] = hi.view(x.shape[0], -1, 4)
    p[:, :, 1, :] = ((v - hi.float()) * 2048.0).half().view(x.shape[0], -1, 4)
    return p


def other_libs():
    """MIX_LIBS -> {name: loaded library}; the default library stays the one in use."""
    out, main = {}, _lib.lib()
    for item in filter(None, os.environ.get("MIX_LIBS", "").split(",")):
        name, path = item.split(":", 1)
        _lib.LIB_PATH, _lib._LIB = os.path.abspath(path), None
        out[name] = _lib.lib()
    _lib._LIB = main
    return out, main


def with_lib(L, main, f):
    def run():
        _lib._LIB = L
        try:
            f()
        finally:
            _lib._LIB = main
    return run


def alternate(forms):
    """forms: name -> callable; the median and the spread of each, alternating."""
    res = {k: [] for k in forms}
    for f in forms.values():  # warm-up (kernel attributes, first launches)
        timed(f, 3)
    for _ in range(ROUNDS):
        for k, f in forms.items():
            res[k].append(timed(f))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


M = int(sys.argv[1]) if len(sys.argv) > 1 else 419430
s = float(2 ** (M.bit_length() - 1))
for N, K in ((264, 264), (264, 460)):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    dy = torch.randn(M, N, device="cuda", generator=g) / M
    x = torch.randn(M, K, device="cuda", generator=g)
    planes = x3.x2p_ok(M, N, K)  # (k_wgrad_tr has the 264 x 264 layers' blocks only)
    mixed = x3.x2p_dy_ok(M, N, K)  # (k_wgrad_mix has the 264 x 460 layer's blocks only)
    dyp = to_planes(dy, s) if planes or mixed else None
    xp = to_planes(x) if planes else None
    out = torch.empty(N, K, device="cuda")

    def algo(name):
        def f():
            x3.set_wgrad_algo(name)
            x3.wgrad(dy, x, prec="x2", dscale=s, out=out)
        return f

    forms = {"dma": algo("dma"), "reg": algo("reg")}
    if planes:
        forms["tr"] = lambda: x3.wgrad(dyp, xp, prec="x2", dscale=1.0, cscale=1.0 / s, out=out, nk=(N, K))
    if mixed:
        def mix():
            x3.wgrad(dyp, x, prec="x2", dscale=1.0, cscale=1.0 / s, out=out, nk=(N, K))

        forms["mix"] = mix
        libs, main = other_libs()
        for name, L in libs.items():
            if hasattr(L, "mm_gemm_x2p_dy_ok"):
                forms["mix_" + name] = with_lib(L, main, mix)
            else:
                forms["dma_" + name] = with_lib(L, main, algo("dma"))
    r = alternate(forms)
    x3.set_wgrad_algo("dma")
    byt = 4.0 * M * (N + K)
    line = {"M": M, "N": N, "K": K}
    for name, (med, lo, hi) in r.items():
        line[name + "_us"] = round(med, 1)
        line[name + "_range_us"] = [round(lo, 1), round(hi, 1)]
        line[name + "_TBps"] = round(byt / med / 1e6, 3)
    line["speedup"] = round(line["reg_us"] / line["dma_us"], 3)
    if planes:
        line["tr_speedup"] = round(line["dma_us"] / line["tr_us"], 3)
    if mixed:
        line["mix_speedup"] = round(line["dma_us"] / line["mix_us"], 3)
    print(json.dumps(line), flush=True)
    del dy, x, dyp, xp

# the 264 x 264 GEMMs: forward (bias, ReLU, bits) and input gradient (bits, column sums)
N = K = 264
g = torch.Generator(device="cuda").manual_seed(1)
a = torch.relu(torch.randn(M, K, device="cuda", generator=g))
ap = to_planes(a)
dy = torch.randn(M, K, device="cuda", generator=g) / M
dyp = to_planes(dy, s)
w = x3.pack(torch.randn(N, K, device="cuda", generator=g) * 0.1, prec="x2")
wt = x3.pack(torch.randn(K, N, device="cuda", generator=g) * 0.1, trans=True, prec="x2")
b = torch.randn(N, device="cuda", generator=g)
mb = x3.mbits(M, "cuda").zero_()
cs = x3.colsum_buf(M, N, "cuda")
o32 = torch.empty(M, N, device="cuda")
op = x3.planes(M, N, "cuda")
r = alternate({
    "fwd_f32_f32": lambda: x3.gemm(a, w, bias=b, relu=True, mbits_out=mb, out=o32),
    "fwd_f32_planes": lambda: x3.gemm(a, w, bias=b, relu=True, mbits_out=mb, out=op),
    "fwd_planes_f32": lambda: x3.gemm(ap, w, bias=b, relu=True, mbits_out=mb, out=o32),
    "fwd_planes_planes": lambda: x3.gemm(ap, w, bias=b, relu=True, mbits_out=mb, out=op),
})
x3.gemm(a, w, bias=b, relu=True, mbits_out=mb, out=o32)
r.update(alternate({
    "bwd_f32_f32": lambda: x3.gemm(dy, wt, mbits_in=mb, colsum=cs, ascale=s, out=o32),
    "bwd_planes_f32": lambda: x3.gemm(dyp, wt, mbits_in=mb, colsum=cs, ascale=1.0, cscale=1.0 / s, out=o32),
    "bwd_planes_planes": lambda: x3.gemm(dyp, wt, mbits_in=mb, colsum=cs, ascale=1.0, cscale=1.0 / s, out=op,
                                         oscale=s),
}))
line = {"M": M, "N": N, "K": K, "gemm": "A_C storage"}
for name, (med, lo, hi) in r.items():
    line[name + "_us"] = round(med, 1)
    line[name + "_range_us"] = [round(lo, 1), round(hi, 1)]
print(json.dumps(line), flush=True)
