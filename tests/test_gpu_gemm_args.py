"""Argument handling of the row-major-A GEMM entries (mm_gemm_nt_h, mm_gemm_nt, mm_x3_nt_f32a): one literal
table of argument sets with the status each returns.  Every rule of the entry's validation appears from both
sides: an accepted set (status 0) next to the sets that break it (MM_E_ARG).  Accepted sets run at 33 rows (the
streaming kernel) or 16,417 (the B-resident kernel's row threshold plus a ragged tile), and where a stored form
(x2 planes, fp16 rows) has an fp32-form twin -- the same call on the fp32 values -- the outputs are compared bit
for bit: the stored forms hold exactly what the kernel's own conversion of the fp32 values gives."""
import ctypes

import pytest
import torch

from marlmaze import _lib, x3

pytestmark = pytest.mark.gpu

E = -1  # MM_E_ARG
A16, C16, AP, CP = _lib.GEMM_A_F16, _lib.GEMM_C_F16, _lib.GEMM_A_X2P, _lib.GEMM_C_X2P
BIG = 16417

# fields (defaults): entry "h" (mm_gemm_nt_h) / "nt" (mm_gemm_nt) / "f32a" (mm_x3_nt_f32a); prec "x2"; flags 0;
# M 33; N 264; K 264; lda K; ldc N; a_off / c_off 0 (bytes added to the pointers); ascale, cscale, oscale 1;
# bias, relu False; bits None / "in" / "out" / "both"; colsum False; algo "auto" / "stream"; a / c "ok" / None
# (a null pointer); f32a only: mask False, ldm N, ctp False.  twin: compare with the fp32-form call.
CASES = [
    # ---- the fp32 form: precision, scales, flags ----
    ("x2 plain", dict(), 0),
    ("x3 plain", dict(prec="x3"), 0),
    ("f16 scaled", dict(prec="f16", ascale=4.0, cscale=0.25), 0),
    ("x3 ascale", dict(prec="x3", ascale=2.0), E),
    ("x3 cscale", dict(prec="x3", cscale=0.5), E),
    ("unknown precision", dict(prec=7), E),
    ("unknown flag bit", dict(flags=64), E),
    ("unknown flag bit beside a known one", dict(flags=CP | 128, bits="out"), E),
    ("mm_gemm_nt", dict(entry="nt"), 0),
    ("mm_gemm_nt null c", dict(entry="nt", c=None), E),
    ("null c", dict(c=None), E),
    ("null a", dict(a=None), E),
    ("lda < K", dict(lda=260), E),
    ("ldc < N", dict(ldc=260), E),
    ("c off by 2 bytes", dict(c_off=2), E),
    # ---- fp32 A rows: 16-byte, 8-byte (narrow outputs only), neither ----
    ("8-byte-aligned a, N <= 64", dict(N=64, a_off=8), 0),
    ("8-byte-aligned a, N > 64", dict(a_off=8), E),
    ("4-byte-aligned a", dict(N=64, a_off=4), E),
    ("K = 130, N = 64", dict(N=64, K=130), 0),
    ("K = 130, N = 64, B-resident", dict(M=BIG, N=64, K=130), 0),
    ("K = 130, N = 264", dict(K=130), E),
    ("odd K", dict(N=64, K=131, lda=132), E),
    ("odd lda", dict(N=64, K=130, lda=131), E),
    # ---- ReLU bits and column sums ----
    ("forward with bits", dict(bits="out", bias=True, relu=True), 0),
    ("input gradient with bits and column sums", dict(bits="in", colsum=True), 0),
    ("both bit masks", dict(bits="both"), E),
    ("bits, N > 272", dict(N=288, bits="out"), E),
    ("bits in with bias", dict(bits="in", bias=True), E),
    ("bits in with ReLU", dict(bits="in", relu=True), E),
    ("column sums without bits in", dict(colsum=True), E),
    ("column sums with bits out", dict(bits="out", colsum=True), E),
    # ---- M = 0 ----
    ("M = 0, fp32", dict(M=0), 0),
    ("M = 0, plane A with bits", dict(M=0, flags=AP, bits="out"), 0),
    ("M = 0, plain plane A", dict(M=0, flags=AP), E),
    ("M = 0, plane C", dict(M=0, flags=CP, bits="out"), 0),
    ("M = 0, fp16 A", dict(M=0, prec="f16", flags=A16), 0),
    ("M = 0, invalid otherwise", dict(M=0, bits="both"), E),
    # ---- x2 plane A ----
    ("plane A, bits, streaming", dict(flags=AP, bits="out", bias=True, relu=True, twin=True), 0),
    ("plane A, bits, B-resident", dict(M=BIG, flags=AP, bits="out", bias=True, relu=True, twin=True), 0),
    ("plane A, bits in, B-resident", dict(M=BIG, flags=AP, bits="in", colsum=True, twin=True), 0),
    ("plain plane A below the row threshold", dict(flags=AP), E),
    ("plain plane A, B-resident", dict(M=BIG, flags=AP, twin=True), 0),
    ("plain plane A, MM_GEMM_STREAM", dict(M=BIG, flags=AP, algo="stream"), E),
    ("plane A with bits, MM_GEMM_STREAM", dict(M=BIG, flags=AP, bits="out", algo="stream", twin=True), 0),
    ("plane A, ascale", dict(flags=AP, bits="out", ascale=2.0), E),
    ("plane A at x3", dict(prec="x3", flags=AP, bits="out"), E),
    ("plane A at f16", dict(prec="f16", flags=AP, bits="out"), E),
    ("plane A, a off by 8", dict(flags=AP, bits="out", a_off=8), E),
    ("plane A, K & 3", dict(flags=AP, bits="out", K=262, lda=264), E),
    ("plane A, lda & 3", dict(flags=AP, bits="out", lda=266), E),
    ("plane A with fp16 A", dict(flags=AP | A16, bits="out"), E),
    ("plane A with fp16 C", dict(flags=AP | C16, bits="out"), E),
    # ---- x2 plane C ----
    ("plane C, forward", dict(flags=CP, bits="out", bias=True, relu=True, twin=True), 0),
    ("plane C, forward, B-resident", dict(M=BIG, flags=CP, bits="out", bias=True, relu=True, twin=True), 0),
    ("plane C, input gradient", dict(M=BIG, flags=CP, bits="in", colsum=True, oscale=4.0, twin=True), 0),
    ("plane A and C", dict(M=BIG, flags=AP | CP, bits="out", bias=True, relu=True, twin=True), 0),
    ("plane C without bits", dict(flags=CP), E),
    ("plane C, N & 3", dict(flags=CP, bits="out", N=262, ldc=264), E),
    ("plane C, ldc & 3", dict(flags=CP, bits="out", ldc=266), E),
    ("plane C, c off by 8", dict(flags=CP, bits="out", c_off=8), E),
    ("plane C, fp32 a off by 8", dict(flags=CP, bits="out", N=64, a_off=8), E),
    ("plane C, K & 3", dict(flags=CP, bits="out", N=64, K=130), E),
    ("plane C at f16", dict(prec="f16", flags=CP, bits="out"), E),
    ("plane C, both bit masks", dict(flags=CP, bits="both"), E),
    ("plane C, bits in with bias", dict(flags=CP, bits="in", bias=True), E),
    ("plane C, column sums without bits in", dict(flags=CP, bits="out", colsum=True), E),
    # ---- fp16 rows ----
    ("fp16 A, B-resident", dict(M=BIG, prec="f16", flags=A16, bits="out", bias=True, relu=True, twin=True), 0),
    ("fp16 A, streaming", dict(prec="f16", flags=A16, bits="out", bias=True, relu=True, twin=True), 0),
    ("fp16 A, plain", dict(prec="f16", flags=A16, twin=True), 0),
    ("fp16 A, ascale", dict(prec="f16", flags=A16, ascale=2.0), E),
    ("fp16 A at x2", dict(flags=A16), E),
    ("fp16 A at x3", dict(prec="x3", flags=A16), E),
    ("fp16 A, a off by 4", dict(prec="f16", flags=A16, a_off=4), E),
    ("fp16 A, a off by 8", dict(prec="f16", flags=A16, a_off=8), 0),
    ("fp16 A, K & 3", dict(prec="f16", flags=A16, K=262, lda=264), E),
    ("fp16 A, lda & 3", dict(prec="f16", flags=A16, lda=266), E),
    ("fp16 C, forward", dict(prec="f16", flags=C16, bits="out", bias=True, relu=True, twin=True), 0),
    ("fp16 C, forward, B-resident", dict(M=BIG, prec="f16", flags=C16, bits="out", bias=True, relu=True, twin=True), 0),
    ("fp16 C, input gradient, B-resident", dict(M=BIG, prec="f16", flags=C16, bits="in", colsum=True, ascale=4.0,
                                                cscale=0.25, oscale=4.0, twin=True), 0),
    ("fp16 C, input gradient below the row threshold", dict(prec="f16", flags=C16, bits="in"), E),
    ("fp16 A and C", dict(M=BIG, prec="f16", flags=A16 | C16, bits="out", bias=True, relu=True, twin=True), 0),
    ("fp16 C without bits", dict(prec="f16", flags=C16), E),
    ("fp16 C at x2", dict(flags=C16, bits="out"), E),
    ("fp16 C, c off by 2", dict(prec="f16", flags=C16, bits="out", c_off=2), E),
    # ---- MM_GEMM_STREAM ----
    ("fp32, MM_GEMM_STREAM", dict(M=BIG, algo="stream"), 0),
    # (no twin: fp16 A takes the B-resident kernel whatever the switch says, its fp32 form then the streaming one)
    ("fp16 A, MM_GEMM_STREAM", dict(M=BIG, prec="f16", flags=A16, bits="out", algo="stream"), 0),
    # ---- mm_x3_nt_f32a: the fp32 mask, the TP output ----
    ("f32a", dict(entry="f32a", prec="x3"), 0),
    ("f32a, mask", dict(entry="f32a", prec="x3", mask=True, bias=True, relu=True), 0),
    ("f32a, mask, ldm < N", dict(entry="f32a", prec="x3", mask=True, ldm=260), E),
    ("f32a, TP output", dict(entry="f32a", prec="x3", ctp=True, c=None), 0),
    ("f32a, neither output", dict(entry="f32a", prec="x3", c=None), E),
    ("f32a, mask with bits", dict(entry="f32a", prec="x3", mask=True, bits="out"), E),
    ("f32a, TP output with bits", dict(entry="f32a", prec="x3", ctp=True, c=None, bits="out"), E),
    ("f32a, a off by 8", dict(entry="f32a", prec="x3", N=64, a_off=8), E),
    ("f32a, K & 3", dict(entry="f32a", prec="x3", N=64, K=130), E),
    ("f32a, bits", dict(entry="f32a", prec="x3", bits="out", bias=True, relu=True), 0),
]

DEFAULTS = dict(entry="h", prec="x2", flags=0, M=33, N=264, K=264, lda=None, ldc=None, a_off=0, c_off=0, ascale=1.0,
                cscale=1.0, oscale=1.0, bias=False, relu=False, bits=None, colsum=False, algo="auto", a="ok", c="ok",
                mask=False, ldm=None, ctp=False, twin=False)
ROWS, WIDTH = BIG, 288  # the shared buffers hold the largest case (and the byte offsets)


def to_planes(x):
    """The x2 planes of an fp32 [M, n] tensor at scale 1 (pair2: hi = fp16(x), lo = fp16(2^11 (x - hi)))."""
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    M, n = x.shape
    return torch.stack((hi.view(M, n // 4, 4), lo.view(M, n // 4, 4)), dim=2).contiguous()


@pytest.fixture(scope="module")
def bufs():
    g = torch.Generator(device="cuda").manual_seed(1109)
    b = dict(
        x=torch.randn(ROWS, WIDTH, device="cuda", generator=g),
        w=torch.randn(WIDTH, WIDTH, device="cuda", generator=g) * 0.05,
        bias=torch.randn(WIDTH, device="cuda", generator=g),
        mask=torch.randn(ROWS, WIDTH, device="cuda", generator=g),
    )
    b["bits_src"] = {}
    return b


def a_tensor(bufs, o):
    """A [M, lda] in the call's form, with room for the byte offset; its fp32 values."""
    M, K, lda = max(o["M"], 1), o["K"], max(o["lda"], o["K"])  # (lda < K is refused: any storage will do)
    vals = torch.zeros(M, lda, device="cuda")
    vals[:, :K] = bufs["x"][:M, :K]
    if o["flags"] & A16:
        vals = vals.half().float()
        store = vals.half()
    elif o["flags"] & AP and lda % 4 == 0:
        store = to_planes(vals)
    else:
        store = vals
    flat = torch.zeros(store.numel() * store.element_size() + 32, dtype=torch.uint8, device="cuda")
    base = flat.data_ptr()
    pad = (-base) % 16 + o["a_off"]
    flat[pad:pad + store.numel() * store.element_size()] = store.view(torch.uint8).reshape(-1)
    return flat, base + pad, vals


def run(bufs, o, fp32_form=False):
    """The call of a case (or of its fp32-form twin): status, output bytes, bit mask, column sums."""
    L = _lib.lib()
    o = dict(o)
    prec = o["prec"] if isinstance(o["prec"], int) else x3.PRECS[o["prec"]]
    M, N, K = o["M"], o["N"], o["K"]
    aflat, aptr, avals = a_tensor(bufs, o)
    flags = o["flags"]
    if fp32_form:  # the same call on the fp32 values, fp32 out
        flags = 0
        aflat = avals.contiguous()
        aptr = aflat.data_ptr()
    wp = x3.pack(bufs["w"][:N, :K].contiguous(), prec={0: "x3", 1: "f16", 2: "x2"}.get(prec, "x2"))
    rows = max(M, 1)
    cbytes = rows * o["ldc"] * 4 + 32
    cflat = torch.zeros(cbytes, dtype=torch.uint8, device="cuda")
    cptr = cflat.data_ptr() + (-cflat.data_ptr()) % 16 + (0 if fp32_form else o["c_off"])
    bits_in = bits_out = None
    if o["bits"] in ("in", "both"):
        key = (rows, N)
        if key not in bufs["bits_src"]:  # a forward's mask of the same [M, N] tiling
            mb = x3.mbits(rows, "cuda")
            x3.gemm(bufs["x"][:rows, :64].contiguous(), x3.pack(bufs["w"][:N, :64].contiguous(), prec="x3"),
                    relu=True, mbits_out=mb)
            bufs["bits_src"][key] = mb
        bits_in = bufs["bits_src"][key]
    if o["bits"] in ("out", "both"):
        bits_out = x3.mbits(rows, "cuda").zero_()
    cs = x3.colsum_buf(rows, N, "cuda").zero_() if o["colsum"] else None
    bias = bufs["bias"][:N].contiguous() if o["bias"] else None
    a = ctypes.c_void_p(aptr) if o["a"] else None
    c = ctypes.c_void_p(cptr) if o["c"] else None
    prev = x3.set_algo(o["algo"])
    try:
        if o["entry"] == "h":
            rc = L.mm_gemm_nt_h(prec, flags, a, o["lda"], o["ascale"], wp.ptr(), M, N, K, _lib.ptr(bias),
                                int(o["relu"]), _lib.ptr(bits_in), _lib.ptr(bits_out), _lib.ptr(cs), o["cscale"],
                                1.0 if fp32_form else o["oscale"], c, o["ldc"], _lib.stream_ptr())
        elif o["entry"] == "nt":
            rc = L.mm_gemm_nt(prec, a, o["lda"], o["ascale"], wp.ptr(), M, N, K, _lib.ptr(bias), int(o["relu"]),
                              _lib.ptr(bits_in), _lib.ptr(bits_out), _lib.ptr(cs), o["cscale"], c, o["ldc"],
                              _lib.stream_ptr())
        else:
            mask = bufs["mask"][:rows, :o["ldm"]].contiguous() if o["mask"] else None
            ctp = x3.TP(rows, N, "cuda") if o["ctp"] else None
            rc = L.mm_x3_nt_f32a(a, o["lda"], wp.ptr(), M, N, K, _lib.ptr(bias), int(o["relu"]), _lib.ptr(mask),
                                 o["ldm"], _lib.ptr(bits_in), _lib.ptr(bits_out), _lib.ptr(cs), c, o["ldc"],
                                 ctp.ptr() if ctp else None, _lib.stream_ptr())
    finally:
        x3.set_algo(prev)
    torch.cuda.synchronize()
    off = cptr - cflat.data_ptr()
    return rc, cflat[off:off + rows * o["ldc"] * 4], bits_out, cs


@pytest.mark.parametrize("name,over,status", CASES, ids=[c[0] for c in CASES])
def test_gemm_argument_set(bufs, name, over, status):
    assert set(over) <= set(DEFAULTS), name
    o = dict(DEFAULTS, **over)
    o["lda"] = o["K"] if o["lda"] is None else o["lda"]
    o["ldc"] = o["N"] if o["ldc"] is None else o["ldc"]
    o["ldm"] = o["N"] if o["ldm"] is None else o["ldm"]
    rc, out, bits, cs = run(bufs, o)
    assert rc == status, f"{name}: status {rc}, expected {status}"
    if status != 0 or not o["twin"] or o["M"] == 0:
        return
    rc32, out32, bits32, cs32 = run(bufs, o, fp32_form=True)
    assert rc32 == 0, name
    M, N, ldc = o["M"], o["N"], o["ldc"]
    ref = out32.view(torch.float32).view(M, ldc)[:, :N]
    if o["flags"] & CP:  # the planes of what the fp32 form stores (times oscale for the input gradient)
        got = out.view(torch.float16).view(M, ldc // 4, 2, 4)[:, :N // 4]
        assert torch.equal(got.view(torch.int16), to_planes(ref * o["oscale"]).view(torch.int16)), name
    elif o["flags"] & C16:
        got = out.view(torch.float16)[:M * ldc].view(M, ldc)[:, :N]
        assert torch.equal(got.view(torch.int16), (ref * o["oscale"]).half().view(torch.int16)), name
    else:
        assert torch.equal(out.view(torch.int32), out32.view(torch.int32)), name
    if bits is not None:
        assert torch.equal(bits, bits32), name
    if cs is not None:
        assert torch.equal(cs.view(torch.int32), cs32.view(torch.int32)), name
