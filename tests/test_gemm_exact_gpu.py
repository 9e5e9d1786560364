"""Every GEMM route against a float64 reference on exact-arithmetic inputs (tests/gemm_ref.py): fp32 outputs bit for
bit, bf16 outputs the bit-exact RNE rounding, GELU epilogues per element to 2^-12.  A and W carry NaN poison around
them, every output has sentinel pad columns (ldc > N) and one row past M that must stay untouched.

Routes are the branches of launch_tile (csrc/gemm_tile.hip), launch_gemv_pro / launch_gemv_tiles / launch_gemv_cpw and
dispatch_gemv13 (csrc/gemm_gemv.hip) and launch_gemv8 (csrc/gemm_gemv8.hip); tile_route / gemv_cpw below restate the
launchers' arithmetic and every case asserts the route its id names.

Out of scope (their values depend on the last bf16 step of h, or on exp): mx_out, amax_out and pro_modes 2-5 -- so of
the six forms in dispatch_gemv13 (QKV_ROPE / pro_mode 1, FX_ADD / 2, FX_ADD / 0, F32_FIN / 0, BF16_GELU_MUL / 1,
F32 / 4) the two with pro_mode 2 and 4 stay with the bit-identity tests of test_frag13_gpu.py and test_frag12_gpu.py.

A HIP error (not a failed assertion) in any case here ends the whole pytest session with return code 3
(_stop_on_device_error): nothing more is launched on a device that has faulted."""
import functools

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

SENT = 123.0            # sentinel of every output pad (bf16-exact)
CUS = 256               # PG_G256_MIN_TILES and the workgroup counts launch_tile compares with


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """A HIP error (not a failed assertion) ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


def cu(t):
    return None if t is None else t.cuda()


def fargs(ops, **kw):
    """ops.fused_args keeps only the addresses of the tensors it is given: return them with it, to be held until the
    launch is enqueued (a temporary freed before that may be handed to the next allocation)."""
    return ops.fused_args(**kw), kw


def ref_dev(p, bias=True):
    """The float64 reference product on the device (exact: every partial sum is a small dyadic number)."""
    out = p.A64.cuda() @ p.W64.cuda().t()
    if bias and getattr(p, "bias64", None) is not None:
        out = out + p.bias64.cuda()
    return out


def padded(rows, N, dtype, lead=None, fill=SENT):
    """A sentinel-filled [rows + 1][N + 8] buffer and its [rows][N] view (or [lead][rows / lead][N]): ldc > N."""
    buf = torch.full((rows + 1, N + 8), fill, dtype=dtype, device="cuda")
    v = buf[:rows]
    if lead:
        v = v.view(lead, rows // lead, N + 8)
    return buf, v[..., :N]


def pads_untouched(buf, rows, N, fill=SENT):
    torch.cuda.synchronize()
    assert bool((buf[:rows, N:] == fill).all()) and bool((buf[rows:] == fill).all()), "a store outside [M][N]"


def ceil(a, b):
    return -(-a // b)


def tile_route(M, N, ks, flags, f32_slabs, fp8=False, mx=False):
    """launch_tile's choice (csrc/gemm_tile.hip), restated."""
    if flags & 0x800:
        return "t64x64-flag"
    if flags & 0x400 and not fp8:
        return "m1-256" if M <= 256 else "m1-288"
    if fp8 and mx:
        return "t128x128-mx"
    t256 = ceil(M, 256) * ceil(N, 256)
    if (not fp8 or f32_slabs) and t256 * ks >= CUS and (ks == 1 or f32_slabs):
        return "g256"
    tiles_n = ceil(N, 128)
    if ceil(M, 128) * tiles_n >= 256:
        return "t128x128"
    if not fp8 and ceil(M, 64) * tiles_n * ks < 256:
        return "t64x64-auto"
    return "t64x128"


def gemv_cpw(K, ks):
    """launch_gemv_tiles' chunks-per-wave specialisation: 4, 8 or 16 when every wave of every split owns that many
    64-element chunks, 0 = the runtime chunk loop."""
    nch = K // 64
    cpw = nch // ks // 4 if nch % ks == 0 and (nch // ks) % 4 == 0 else 0
    return cpw if cpw in (4, 8, 16) else 0


# ------------------------------------------------------------------------------------------ tile GEMMs, bf16 operands
# id -> (M, N, flags, route).  TBN = 128, m64 = ceil(M / 64), tiles_n = ceil(N / 128), t128 = ceil(M / 128) * tiles_n,
# t256 = ceil(M / 256) * ceil(N / 256):
#   17 x 192:    m64 * tiles_n = 1 * 2 = 2 < 256                                   -> 64 x 64, auto
#   17 x 300:    1 * 3 = 3;  100 x 192: 2 * 2 = 4;  100 x 300: 2 * 3 = 6           -> 64 x 64, auto
#   300 x 704:   PG_TILE_N64                                                        -> 64 x 64, flag
#   520 x 3712:  m64 * tiles_n = 9 * 29 = 261 >= 256, t128 = 5 * 29 = 145 < 256, t256 = 3 * 15 = 45 -> 64 x 128, 8 waves
#   1100 x 3712: t128 = 9 * 29 = 261 >= 256, t256 = 5 * 15 = 75 < 256              -> 128 x 128
#   4113 x 3856: t256 = ceil(4113 / 256) * ceil(3856 / 256) = 17 * 16 = 272 >= PG_G256_MIN_TILES -> 256 x 256
#   256 / 264 / 288 x 384 with PG_TILE_M1: the 256-row form at M <= 256, the 288-row form above
TILE_CASES = {
    "t64x64-auto-M17-N192": (17, 192, 0, "t64x64-auto"),
    "t64x64-auto-M17-N300": (17, 300, 0, "t64x64-auto"),
    "t64x64-auto-M100-N192": (100, 192, 0, "t64x64-auto"),
    "t64x64-auto-M100-N300": (100, 300, 0, "t64x64-auto"),
    "t64x64-flag-M300-N704": (300, 704, 0x800, "t64x64-flag"),
    "t64x128-M520-N3712": (520, 3712, 0, "t64x128"),
    "t128x128-M1100-N3712": (1100, 3712, 0, "t128x128"),
    "g256-M4113-N3856": (4113, 3856, 0, "g256"),
    "m1-M256-N384": (256, 384, 0x400, "m1-256"),
    "m1-M264-N384": (264, 384, 0x400, "m1-288"),
    "m1-M288-N384": (288, 384, 0x400, "m1-288"),
}
RAGGED_KS = {64: 2, 192: 2, 320: 3}     # k-tiles 1 + 0, 2 + 1, 2 + 2 + 1


def _f32_slabs(ops, A, W, bias, M, N, ks, epi):
    buf, out = padded(ks * M, N, torch.float32, lead=ks)
    ops.gemm(A, W, out, epi=epi, bias=bias, ksplit=ks, M=M, N=N)
    pads_untouched(buf, ks * M, N)
    return out


@pytest.mark.parametrize("K", [64, 192, 320])
@pytest.mark.parametrize("case", list(TILE_CASES))
def test_tile_routes_exact(case, K):
    """Each tile route (table above) at one, three and five k-tiles (fewer than, and more than, the pipeline has
    stages), row-major and fragment-packed W: EPI_BF16 + bias, EPI_F32 at ks 1 and a ragged ks (the slab sum; a launch
    without bias shows the bias entered once), EPI_F32_RES on an integer residual; EPI_F32_POS and EPI_BF16_VT on the
    64-row routes."""
    from pghip import ops
    from pghip.weights import frag_pack
    M, N, flags, route = TILE_CASES[case]
    ks = RAGGED_KS[K]
    assert tile_route(M, N, 1, flags, False) == route and ops.finalize_split(M, N, K) == 1
    assert tile_route(M, N, ks, flags, True) == route          # the ragged-ks EPI_F32 launch stays on the route
    p = R.exact_pair(M, N, K, seed=1000 + K)
    A, W = R.poisoned(cu(p.A), cu(p.W))
    bias = cu(p.bias)
    ref0 = ref_dev(p, bias=False)
    ref = ref0 + cu(p.bias64)
    resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(K)).double().cuda()
    layouts = [("row", W, 0)]
    if N % 16 == 0:
        layouts.append(("frag", frag_pack(cu(p.W)), ops.W_FRAG))
    for name, Wl, lf in layouts:
        f = flags | lf
        buf, out = padded(M, N, torch.bfloat16)
        ops.gemm(A, Wl, out, epi=ops.EPI_BF16 | f, bias=bias, M=M, N=N)
        R.assert_all(R.exact_bf16(out, ref), f"{case} {name} BF16")
        pads_untouched(buf, M, N)
        for s in (1, ks):
            part = _f32_slabs(ops, A, Wl, bias, M, N, s, ops.EPI_F32 | f)
            R.assert_all(R.exact_f32(part.sum(0), ref), f"{case} {name} F32 ks {s}")
            part0 = _f32_slabs(ops, A, Wl, None, M, N, s, ops.EPI_F32 | f)
            R.assert_all(R.exact_f32(part0.sum(0), ref0), f"{case} {name} F32 ks {s}, no bias")
            if s > 1:                                        # the bias is in slab 0 alone
                assert torch.equal(part[1:], part0[1:]) and torch.equal(part[0] - part0[0], bias.expand(M, N))
        buf, out = padded(M, N, torch.float32)
        out.copy_(resid64.float())
        ops.gemm(A, Wl, out, epi=ops.EPI_F32_RES | f, bias=bias, M=M, N=N)
        R.assert_all(R.exact_f32(out, resid64 + ref), f"{case} {name} F32_RES")
        pads_untouched(buf, M, N)
    if route.startswith("t64"):
        # EPI_F32_POS: C = acc + bias + aux[m % aux_rows] (aux rows share C's stride); row-major W only
        buf, out = padded(M, N, torch.float32)
        auxb, aux = padded(8, N, torch.float32)
        aux64 = torch.randint(-64, 65, (8, N), generator=torch.Generator().manual_seed(K + 1)).double().cuda()
        aux.copy_(aux64.float())
        ops.gemm(A, W, out, epi=ops.EPI_F32_POS | flags, bias=bias, aux=auxb, aux_rows=8, M=M, N=N)
        R.assert_all(R.exact_f32(out, ref + aux64[torch.arange(M, device="cuda") % 8]), f"{case} F32_POS")
        pads_untouched(buf, M, N)
        # EPI_BF16_VT: columns < aux_n to C, the rest transposed into aux_out
        aux_n = (2 * N // 3) // 4 * 4
        buf, out = padded(M, N, torch.bfloat16)
        vtb, vt = padded(N - aux_n, M, torch.bfloat16)
        ops.gemm(A, W, out, epi=ops.EPI_BF16_VT | flags, bias=bias, aux_out=vtb, aux_ld=M + 8, aux_n=aux_n, M=M, N=N)
        R.assert_all(R.exact_bf16(out[:, :aux_n].contiguous(), ref[:, :aux_n].contiguous()), f"{case} VT head")
        R.assert_all(R.exact_bf16(vt.contiguous(), ref[:, aux_n:].t().contiguous()), f"{case} VT tail")
        assert bool((out[:, aux_n:] == SENT).all())
        pads_untouched(buf, M, N)
        pads_untouched(vtb, N - aux_n, M)


def test_tile_g256_split_k_ragged():
    """The 256 x 256 kernel with a K split: 2100 x 2320, K 320, ks 3 -- t256 * ks = 9 * 10 * 3 = 270 >=
    PG_G256_MIN_TILES with EPI_F32 (kts = ceil(5 / 3) = 2: k-tiles 2, 2, 1); at ks 1 the same shape is a 128 x 128
    grid (t128 = 17 * 19 = 323)."""
    from pghip import ops
    from pghip.weights import frag_pack
    M, N, K, ks = 2100, 2320, 320, 3
    assert tile_route(M, N, ks, 0, True) == "g256" and tile_route(M, N, 1, 0, True) == "t128x128"
    p = R.exact_pair(M, N, K, seed=77)
    A, W = R.poisoned(cu(p.A), cu(p.W))
    ref0 = ref_dev(p, bias=False)
    for name, Wl, lf in (("row", W, 0), ("frag", frag_pack(cu(p.W)), ops.W_FRAG)):
        part = _f32_slabs(ops, A, Wl, cu(p.bias), M, N, ks, ops.EPI_F32 | lf)
        R.assert_all(R.exact_f32(part.sum(0), ref0 + cu(p.bias64)), f"g256 ks 3 {name}")
        # each slab holds its own k-tiles: 0..127, 128..255, 256..319
        for z, (k0, k1) in enumerate(((0, 128), (128, 256), (256, 320))):
            want = p.A64[:, k0:k1].cuda() @ p.W64[:, k0:k1].cuda().t() + (cu(p.bias64) if z == 0 else 0)
            R.assert_all(R.exact_f32(part[z].contiguous(), want), f"g256 ks 3 {name} slab {z}")


@pytest.mark.parametrize("M,N", [(100, 300), (264, 704)])
def test_finalize_split_both_ways_exact(M, N):
    """ops.gemm's own split + pg_gemm_finalize for the bf16 epilogues (finalize_split: 64 x 128 tiles 2 * 3 = 6 and
    5 * 6 = 30 <= 100, K / 64 = 12 >= 12 -> 2 splits) and the one-launch epilogue with the switch off: both exact."""
    from pghip import ops
    K = 768
    assert ops.finalize_split(M, N, K) == 2
    p = R.exact_pair(M, N, K, seed=31)
    A, W = R.poisoned(cu(p.A), cu(p.W))
    ref = ref_dev(p)
    aux_n = (2 * N // 3) // 4 * 4
    for split in (True, False):
        ops.FINALIZE_SPLIT = split
        try:
            assert (ops.finalize_split(M, N, K) > 1) == split
            buf, out = padded(M, N, torch.bfloat16)
            ops.gemm(A, W, out, epi=ops.EPI_BF16, bias=cu(p.bias))
            buf2, out2 = padded(M, N, torch.bfloat16)
            vtb, vt = padded(N - aux_n, M, torch.bfloat16)
            ops.gemm(A, W, out2, epi=ops.EPI_BF16_VT, bias=cu(p.bias), aux_out=vtb, aux_ld=M + 8, aux_n=aux_n)
        finally:
            ops.FINALIZE_SPLIT = True
        R.assert_all(R.exact_bf16(out, ref), f"BF16 split {split}")
        R.assert_all(R.exact_bf16(out2[:, :aux_n].contiguous(), ref[:, :aux_n].contiguous()), f"VT head {split}")
        R.assert_all(R.exact_bf16(vt.contiguous(), ref[:, aux_n:].t().contiguous()), f"VT tail split {split}")
        assert bool((out2[:, aux_n:] == SENT).all())
        for b, r, n in ((buf, M, N), (buf2, M, N), (vtb, N - aux_n, M)):
            pads_untouched(b, r, n)


# ------------------------------------------------------------------------------------------ GEMV (M <= 16), bf16
GEMV_K = [(64, 1), (192, 1), (1024, 1), (2048, 1), (4096, 1), (4096, 4), (2048, 3)]
GEMV_CPW = {(64, 1): 0, (192, 1): 0, (1024, 1): 4, (2048, 1): 8, (4096, 1): 16, (4096, 4): 4, (2048, 3): 0}


def _gemv_fin(ops, M, N, K, ks, frag, seed, use_fx):
    """PG_EPI_F32_FIN: fin_resid = resid (or fx) + acc + bias, ss_out = its sum of squares per 16-column tile (M <= 4:
    one tile per workgroup) or per tile pair (M > 4: two), fin_x = bf16(fin_resid * (1 + w)), tickets left zero, fx
    cleared.  amp 1 and W * 2^-3 keep |fin_resid| <= 64 on a 2^-3 grid, so the 32-column sums of squares are exact."""
    from pghip.weights import frag_pack
    p = R.exact_pair(M, N, K, seed, amp=1, w_shift=False, w_exp=-3, bias_max=4.0)
    g = torch.Generator().manual_seed(seed + 1)
    resid64 = (torch.randint(-32, 33, (M, N), generator=g).double() * 0.25).cuda()
    w1 = torch.tensor(R.NORM_W1, dtype=torch.float64)[torch.randint(0, 4, (N,), generator=g)].cuda()
    ref = resid64 + ref_dev(p)
    assert float(ref.abs().max()) <= 64
    A, W = R.poisoned(cu(p.A), cu(p.W))
    Wl = frag_pack(cu(p.W)) if frag else W
    tiles = ceil(N, 16)
    nss = tiles if M <= 4 else ceil(tiles, 2)
    part = torch.full((ks * M + 1, N), SENT, device="cuda")
    res = torch.full((M + 1, N), SENT, device="cuda")
    xq = torch.full((M + 1, N), SENT, dtype=torch.bfloat16, device="cuda")
    ssb = torch.full((M + 1, tiles + 8), SENT, device="cuda")          # (ss_ld >= ceil(N / 16) is required)
    cnt = torch.zeros(tiles, dtype=torch.int32, device="cuda")
    fx = None
    if use_fx:
        fx = torch.zeros(M + 1, N, dtype=torch.int64, device="cuda")
        fx[:M] = (resid64 * 2.0 ** 32).to(torch.int64)
        fx[M] = 12345
    else:
        res[:M] = resid64.float()
    fa, held = fargs(ops, fin_cnt=cnt, fin_resid=res, ss_out=ssb, ss_ld=tiles + 8, fin_x=xq,
                     norm_w=(w1 - 1).float(), fx=fx)
    ops.gemm_fused(A, Wl, part[:ks * M].view(ks, M, N), fa, epi=ops.EPI_F32_FIN | (ops.W_FRAG if frag else 0), M=M,
                   ksplit=ks, bias=cu(p.bias), N=N, ldc=N)
    torch.cuda.synchronize()
    what = f"FIN M {M} N {N} K {K} ks {ks} frag {frag} fx {use_fx}"
    R.assert_all(R.exact_f32(res[:M], ref), what + " fin_resid")
    R.assert_all(R.exact_bf16(xq[:M], ref * w1), what + " fin_x")
    sq = torch.zeros(M, tiles * 16, dtype=torch.float64, device="cuda")
    sq[:, :N] = ref * ref
    want_ss = sq.view(M, tiles, 16).sum(-1)
    if M > 4:
        want_ss = torch.cat([want_ss, want_ss.new_zeros(M, 2 * nss - tiles)], 1).view(M, nss, 2).sum(-1)
    R.assert_all(R.exact_f32(ssb[:M, :nss].contiguous(), want_ss), what + " ss_out")
    assert bool((ssb[:M, nss:] == SENT).all()) and bool((ssb[M] == SENT).all())
    assert int(cnt.abs().sum()) == 0 and bool((res[M] == SENT).all()) and bool((xq[M] == SENT).all())
    assert bool((part[ks * M] == SENT).all())
    if use_fx:
        assert int(fx[:M].abs().sum()) == 0 and bool((fx[M] == 12345).all())


@pytest.mark.parametrize("K,ks", GEMV_K)
@pytest.mark.parametrize("M", [1, 3, 4, 5, 16])
def test_gemv_routes_exact(M, K, ks):
    """The bf16 weight-streaming GEMV: one 16-row tile per workgroup at M <= 4, two at M > 4 (launch_gemv_pro), N 48 and
    304 = 3 and 19 tiles, so two-tile workgroups get an odd last tile, and N 300 (row-major only: a ragged last tile).
    K x ks picks launch_gemv_cpw's form, nch = K / 64 chunks: (64, 1) and (192, 1) 1 and 3 chunks -> the runtime chunk
    loop; (1024, 1) 16 / 4 waves -> CPW 4; (2048, 1) CPW 8; (4096, 1) CPW 16; (4096, 4) 16 chunks a split -> CPW 4
    through a split; (2048, 3) 32 % 3 != 0 -> a ragged split on the runtime loop.  Epilogues: BF16 (ks 1), F32 slabs,
    F32_ADD and FX_ADD onto an integer residual (any atomic order is exact; FX also with resid_in), F32_FIN."""
    from pghip import ops
    from pghip.weights import frag_pack
    assert gemv_cpw(K, ks) == GEMV_CPW[(K, ks)]
    for N, frag in ((48, False), (48, True), (304, False), (304, True), (300, False)):
        p = R.exact_pair(M, N, K, seed=K + 13 * N + M)
        A, W = R.poisoned(cu(p.A), cu(p.W))
        Wl, lf = (frag_pack(cu(p.W)), ops.W_FRAG) if frag else (W, 0)
        bias = cu(p.bias)
        ref = ref_dev(p)
        what = f"M {M} N {N} K {K} ks {ks} frag {frag}"
        if ks == 1:
            buf, out = padded(M, N, torch.bfloat16)
            ops.gemm(A, Wl, out, epi=ops.EPI_BF16 | lf, bias=bias, M=M, N=N)
            R.assert_all(R.exact_bf16(out, ref), what + " BF16")
            pads_untouched(buf, M, N)
        part = _f32_slabs(ops, A, Wl, bias, M, N, ks, ops.EPI_F32 | lf)
        R.assert_all(R.exact_f32(part.sum(0), ref), what + " F32 slabs")
        resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(N + K)).double().cuda()
        buf, out = padded(M, N, torch.float32)
        out.copy_(resid64.float())
        ops.gemm_fused(A, Wl, out, ops.fused_args(), epi=ops.EPI_F32_ADD | lf, M=M, ksplit=ks, bias=bias, N=N)
        R.assert_all(R.exact_f32(out, resid64 + ref), what + " F32_ADD")
        pads_untouched(buf, M, N)
        for rin in (None, resid64.float().contiguous()):
            buf, acc = padded(M, N, torch.int64, fill=12345)
            acc.copy_((resid64 * 2.0 ** 32).to(torch.int64))
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.gemm_fused(A, Wl, acc, ops.fused_args(status=st, resid_in=rin), epi=ops.EPI_FX_ADD | lf, M=M,
                           ksplit=ks, bias=bias, N=N)
            want = ((resid64 * (1 if rin is None else 2) + ref) * 2.0 ** 32).to(torch.int64)
            assert torch.equal(acc, want), what + f" FX_ADD resid_in {rin is not None}"
            pads_untouched(buf, M, N, fill=12345)
            assert int(st) == 0
        for use_fx in ((False, True) if N == 300 else (frag,)):      # (N 300, a ragged last tile: both residual forms)
            _gemv_fin(ops, M, N, K, ks, frag, seed=K + N + M, use_fx=use_fx)


@functools.lru_cache(maxsize=None)
def _lm_head():
    """One full-vocabulary exact weight (131072 x 64), row-major with poison rows and fragment-packed, read-only."""
    from pghip.weights import frag_pack
    p = R.exact_pair(4, 131072, 64, seed=5)
    Wd = cu(p.W)
    _, W = R.poisoned(cu(p.A), Wd)
    return p, W, frag_pack(Wd), cu(p.bias), ref_dev(p)


@pytest.mark.parametrize("M", [1, 4])
def test_gemv_two_tile_lm_head_route_exact(M):
    """launch_gemv_pro's lm_head form: PG_EPI_F32, M <= 4, ceil(131072 / 16) = 8192 >= 8192 tiles, ks 1 -> two tiles per
    workgroup at PG_GEMV_LM_D chunks in flight; K 64 is one chunk (the runtime loop)."""
    from pghip import ops
    p, W, Wf, bias, ref = _lm_head()
    A, _ = R.poisoned(cu(p.A[:M]), cu(p.W[:16]))
    for name, Wl, lf in (("row", W, 0), ("frag", Wf, ops.W_FRAG)):
        part = _f32_slabs(ops, A, Wl, bias, M, p.N, 1, ops.EPI_F32 | lf)
        R.assert_all(R.exact_f32(part[0].contiguous(), ref[:M].contiguous()), f"lm_head M {M} {name}")


@pytest.mark.parametrize("nsplit,use_fx,with_resid", [(0, False, True), (1, False, True), (4, False, True),
                                                      (4, True, True), (0, True, False)])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_gemv_rmsnorm_prologue_exact(M, nsplit, use_fx, with_resid):
    """pro_mode 1 on norm_rows_exact rows: resid_out = resid_in + fx + the first nsplit slabs bit for bit, and because x
    is exactly +-(1 + w) the GEMM behind the norm is exact too (BF16 and F32).  K 2048 (M 1: the register-resident
    row) and K 192."""
    from pghip import ops
    from pghip.weights import frag_pack
    for K, N, frag in ((2048, 304, True), (192, 300, False)):
        n = R.norm_rows_exact(M, K, nsplit, seed=K + M + nsplit, use_fx=use_fx, with_resid=with_resid)
        p = R.exact_pair(M, N, K, seed=K + 3)
        p.A64 = n.x64
        ref = ref_dev(p)
        _, W = R.poisoned(cu(p.A), cu(p.W))
        Wl, lf = (frag_pack(cu(p.W)), ops.W_FRAG) if frag else (W, 0)
        for epi, dt, chk in ((ops.EPI_BF16, torch.bfloat16, R.exact_bf16), (ops.EPI_F32, torch.float32, R.exact_f32)):
            rout = torch.full((M + 1, K), SENT, device="cuda")
            fa, held = fargs(ops, pro_mode=ops.PRO_RMSNORM, resid_in=cu(n.resid), resid_out=rout,
                             partials=cu(n.partials), nsplit=nsplit, norm_w=cu(n.norm_w), eps=1e-6, fx=cu(n.fx))
            buf, out = padded(M, N, dt)
            ops.gemm_fused(None, Wl, out, fa, epi=epi | lf, M=M, bias=cu(p.bias), N=N)
            what = f"pro 1 M {M} K {K} nsplit {nsplit} fx {use_fx} epi {epi}"
            R.assert_all(chk(out, ref), what)
            pads_untouched(buf, M, N)
            R.assert_all(R.exact_f32(rout[:M], cu(n.v64)), what + " resid_out")
            assert bool((rout[M] == SENT).all())


# ------------------------------------------------------------------------------------------ 13- and 12-bit packs
def _packs(W):
    from pghip import ops
    from pghip.weights import frag12_pack, frag13_pack
    p13, p12 = frag13_pack(W), frag12_pack(W)
    assert p13 is not None and p12 is not None
    return (("13", p13, ops.W_FRAG13), ("12", p12, ops.W_FRAG13 | ops.W_FRAG12))


def _wide_blocks(p):
    """Plant a zero and two 2^-20-scaled rows (3 and 11 of every 16: a RoPE pair at D 16) in every 16-row x 128-k
    block, so code 0 and 5-bit (wide) blocks occur.  The scaled rows stay exact -- their sums are small integers times
    2^-23 -- as long as nothing of unit size is added to them: their bias is zero."""
    p.W64 = p.W64.clone()
    for r in (3, 11):
        p.W64[r::16] = p.W64[r::16] * 2.0 ** -20
        if p.bias is not None:
            p.bias64 = p.bias64.clone()
            p.bias64[r::16] = 0.0
            p.bias = p.bias64.float()
    for b in range(p.K // 128):
        p.W64[5::16, 128 * b + (7 * b) % 128] = 0.0
    p.W = p.W64.to(torch.bfloat16)
    assert torch.equal(p.W.double(), p.W64)
    return p


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("K", [1024, 2048])
@pytest.mark.parametrize("M", [1, 4])
def test_packed_decode_forms_exact(M, K, wide):
    """The PG_W_FRAG13 and PG_W_FRAG12 decode forms with pro_mode 0 or 1, against the float64 reference rather than the
    PG_W_FRAG launch: FX_ADD (ks 1 and 2: (K / 64) % (8 ks) == 0) and F32_FIN with plain rows, QKV_ROPE and
    BF16_GELU_MUL behind the RMSNorm prologue.  The exact weights (integers in [-8, 8] times 2^-(n % 4)) span few
    exponents and, with their zeros replaced, hold no exponent field 0, so every block packs narrow; `wide` plants a
    zero and two 2^-20-scaled rows in every block, so every block is wide and holds a code 0."""
    from pghip import ops
    from pghip.weights import frag12_pack, frag12_table
    N = 48
    what = f"M {M} K {K} wide {wide}"
    p = R.exact_pair(M, N, K, seed=K + M, w_nonzero=True)
    if wide:
        p = _wide_blocks(p)
    _, _, wd, _, _ = frag12_table(frag12_pack(cu(p.W)), N, K)
    assert bool(wd.bool().all()) == wide and bool(wd.bool().any()) == wide
    ref = ref_dev(p)
    A, _ = R.poisoned(cu(p.A), cu(p.W))
    resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(K)).double().cuda()
    keep = torch.ones(N, dtype=torch.float64, device="cuda")
    if wide:                                                 # nothing of unit size is added to the scaled rows' sums
        keep[3::16] = 0.0
        keep[11::16] = 0.0
    resid64 = resid64 * keep
    for name, pk, lf in _packs(cu(p.W)):
        for ks in (1, 2):
            buf, acc = padded(M, N, torch.int64, fill=12345)
            acc.copy_((resid64 * 2.0 ** 32).to(torch.int64))
            ops.gemm_fused(A, pk, acc, ops.fused_args(), epi=ops.EPI_FX_ADD | lf, M=M, ksplit=ks, bias=cu(p.bias),
                           N=N, K=K)
            want = (resid64 + ref) * 2.0 ** 32
            # (the 2^-20 row: its products are multiples of 2^-20, times 2^32 still integers)
            assert torch.equal(want, want.round()) and torch.equal(acc, want.to(torch.int64)), what + f" FX {name} {ks}"
            pads_untouched(buf, M, N, fill=12345)
    # F32_FIN: the small-magnitude pair of _gemv_fin
    q = R.exact_pair(M, N, K, seed=K + M + 1, amp=1, w_shift=False, w_exp=-3, bias_max=4.0, w_nonzero=True)
    if wide:
        q = _wide_blocks(q)
    g = torch.Generator().manual_seed(K + 2)
    r64 = (torch.randint(-32, 33, (M, N), generator=g).double() * 0.25).cuda() * keep
    w1 = torch.tensor(R.NORM_W1, dtype=torch.float64)[torch.randint(0, 4, (N,), generator=g)].cuda()
    fref = r64 + ref_dev(q)
    assert float(fref.abs().max()) <= 64
    Aq, _ = R.poisoned(cu(q.A), cu(q.W))
    for name, pk, lf in _packs(cu(q.W)):
        for ks in (1, 2):
            part = torch.full((ks, M, N), SENT, device="cuda")
            res = torch.full((M + 1, N), SENT, device="cuda")
            res[:M] = r64.float()
            xq = torch.full((M + 1, N), SENT, dtype=torch.bfloat16, device="cuda")
            ss = torch.full((M + 1, 3), SENT, device="cuda")
            cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
            fa, held = fargs(ops, fin_cnt=cnt, fin_resid=res, ss_out=ss, ss_ld=3, fin_x=xq, norm_w=(w1 - 1).float())
            ops.gemm_fused(Aq, pk, part, fa, epi=ops.EPI_F32_FIN | lf, M=M, ksplit=ks, bias=cu(q.bias), N=N, K=K)
            torch.cuda.synchronize()
            R.assert_all(R.exact_f32(res[:M], fref), what + f" FIN {name} ks {ks}")
            R.assert_all(R.exact_bf16(xq[:M], fref * w1), what + f" FIN x' {name} ks {ks}")
            if not wide:       # (a 2^-20-scaled row's squares fall off the 2^-6 grid: the sums are no longer exact)
                R.assert_all(R.exact_f32(ss[:M], (fref * fref).view(M, 3, 16).sum(-1)), what + f" FIN ss {name}")
            assert int(cnt.abs().sum()) == 0 and bool((res[M] == SENT).all()) and bool((ss[M] == SENT).all())
    # behind the RMSNorm prologue: gelu(gate) * up (N 96: three tile pairs) and q|k|v with RoPE (D 16, one head each)
    n = R.norm_rows_exact(M, K, 0, seed=K + 5)
    gp = R.gelu_pair(M, 96, K, seed=K + 6, mul=True, A64=n.x64, room=R.GELU_MAX - 1, w_nonzero=True)
    if wide:                                  # (a planted zero moves a pre-activation by less than the room left)
        gp = _wide_blocks(gp)
    href = ref_dev(gp)
    assert float(href.abs().max()) <= R.GELU_MAX
    href = R.gelu_mul64(href)
    for name, pk, lf in _packs(cu(gp.W)):
        buf, h = padded(M, 48, torch.bfloat16)
        fa, held = fargs(ops, pro_mode=ops.PRO_RMSNORM, resid_in=cu(n.resid), nsplit=0, norm_w=cu(n.norm_w), eps=1e-6)
        ops.gemm_fused(None, pk, h, fa, epi=ops.EPI_BF16_GELU_MUL | lf, M=M, N=96, K=K)
        R.assert_all(R.within_bf16(h, href, R.GELU_DELTA), what + f" GELU_MUL {name}")
        pads_untouched(buf, M, 48)
    rp = R.exact_pair(M, 48, K, seed=K + 7, w_nonzero=True)
    rp.bias = rp.bias64 = None
    if wide:
        rp = _wide_blocks(rp)
    rp.A64 = n.x64
    for name, pk, lf in _packs(cu(rp.W)):
        fa_kw = dict(pro_mode=ops.PRO_RMSNORM, resid_in=cu(n.resid), nsplit=0, norm_w=cu(n.norm_w), eps=1e-6)
        _qkv_case(ops, rp, None, pk, lf, M=M, L=1, nh=1, nkv=1, hd=16, smax=32, what=what + f" QKV {name}",
                  fa_kw=fa_kw, extra=dict(N=48, K=K))


# ------------------------------------------------------------------------------------------ GELU, GELU_MUL
def _gelu_checks(ops, M, N, K, flags, what, frag_too=True):
    from pghip.weights import frag_pack
    p = R.gelu_pair(M, N, K, seed=M + N + K)
    A, W = R.poisoned(cu(p.A), cu(p.W))
    buf, out = padded(M, N, torch.bfloat16)
    ops.gemm(A, W, out, epi=ops.EPI_BF16_GELU | flags, bias=cu(p.bias), M=M, N=N)
    R.assert_all(R.within_bf16(out, R.gelu64(ref_dev(p)), R.GELU_DELTA), what + " GELU")
    pads_untouched(buf, M, N)
    if N % 32:
        return
    q = R.gelu_pair(M, N, K, seed=M + N + K + 1, mul=True)
    A, W = R.poisoned(cu(q.A), cu(q.W))
    want = R.gelu_mul64(ref_dev(q))
    for name, Wl, lf in (("row", W, 0), ("frag", frag_pack(cu(q.W)), ops.W_FRAG))[:2 if frag_too else 1]:
        buf, out = padded(M, N // 2, torch.bfloat16)
        ops.gemm(A, Wl, out, epi=ops.EPI_BF16_GELU_MUL | flags | lf, M=M, N=N)
        R.assert_all(R.within_bf16(out, want, R.GELU_DELTA), what + f" GELU_MUL {name}")
        pads_untouched(buf, M, N // 2)


# 150 x 320: 3 * 3 = 9 workgroups -> 64 x 64 auto; 1100 x 3712 -> 128 x 128 and 4113 x 3872 (17 * 16 = 272) -> 256 x 256
# as in TILE_CASES (3872 = 121 * 32 for the gate / up interleave); 264 x 384 with PG_TILE_M1 -> the 288-row form
@pytest.mark.parametrize("M,N,K,flags,route", [(1, 320, 192, 0, "gemv"), (16, 320, 192, 0, "gemv"),
                                               (150, 320, 192, 0, "t64x64-auto"), (1100, 3712, 64, 0, "t128x128"),
                                               (4113, 3872, 64, 0, "g256"), (264, 384, 192, 0x400, "m1-288")])
def test_gelu_epilogues_within_delta(M, N, K, flags, route):
    """EPI_BF16_GELU (+ bias) and EPI_BF16_GELU_MUL on the GEMV (M 1, 16: one and two tiles per workgroup -- GELU_MUL
    always runs the tile pair) and the 64 x 64, 128 x 128, 256 x 256 and PG_TILE_M1 tile routes: every element is the
    bf16 rounding of a value within 2^-12 of the float64 tanh-GELU."""
    from pghip import ops
    if M > 16:
        assert tile_route(M, N, 1, flags, False) == route and ops.finalize_split(M, N, K) == 1
    _gelu_checks(ops, M, N, K, flags, f"{route} M {M} N {N} K {K}")


def test_gelu_epilogues_finalize_route_within_delta():
    """... and through split + pg_gemm_finalize (264 x 704, K 768: 2 splits), with the switch both ways."""
    from pghip import ops
    M, N, K = 264, 704, 768
    assert ops.finalize_split(M, N, K) == 2
    for split in (True, False):
        ops.FINALIZE_SPLIT = split
        try:
            _gelu_checks(ops, M, N, K, 0, f"finalize {split}", frag_too=False)
        finally:
            ops.FINALIZE_SPLIT = True


# ------------------------------------------------------------------------------------------ q|k|v with RoPE
def _qkv_case(ops, p, A, W, lf, *, M, L, nh, nkv, hd, smax, what, slot_rows=False, fa_kw=None, extra=None):
    """One PG_EPI_QKV_ROPE launch on the pair p (its W rows are the packed, rope-permuted order) against qkv_rope_ref
    on the exact accumulators: q, kc, vtc, kd, vd, all exact_bf16; whatever is not written keeps the sentinel."""
    nblk, B = nh + 2 * nkv, M // L
    g = torch.Generator().manual_seed(M + hd)
    pos = torch.randint(0, 48, (M,), generator=g).to(torch.int32)
    cos_t, sin_t = R.rope_tables_exact(48, hd, seed=hd + M)
    slot_base = 3
    if slot_rows:                         # unequal slots per batch row; the last row's lies past the cache
        sd = torch.tensor([(5 + 7 * b) % (smax - L - 3) for b in range(B)], dtype=torch.int32)
        sd[B - 1] = smax
        slots = [slot_base + int(sd[m // L]) + m % L for m in range(M)]
    else:
        sd = torch.tensor([5], dtype=torch.int32)
        slots = [slot_base + 5 + m % L for m in range(M)]
    acc = ref_dev(p, bias=False).cpu().view(M, nblk, hd)
    orig = torch.empty_like(acc)
    orig[:, :, torch.from_numpy(R.rope_row_perm(hd))] = acc            # packed column j holds original dim perm[j]
    want = R.qkv_rope_ref(orig.reshape(M, nblk * hd), pos, cos_t, sin_t, L=L, Hq=nh, Hkv=nkv, D=hd, smax=smax,
                          slots=slots, fill=SENT)
    buf, q = padded(M, nh * hd, torch.bfloat16)
    kc = torch.full((B, smax, nkv * hd), SENT, dtype=torch.bfloat16, device="cuda")
    vtc = torch.full((B, nkv * hd, smax), SENT, dtype=torch.bfloat16, device="cuda")
    kd = torch.full((B, nkv, smax, hd), SENT, dtype=torch.bfloat16, device="cuda")
    vd = torch.full_like(kd, SENT)
    fa, held = fargs(ops, head_dim=hd, cos_t=cu(cos_t), sin_t=cu(sin_t), pos=cu(pos), rows_per_batch=L,
                     slot_dev=cu(sd), slot_base=slot_base, kc=kc, vtc=vtc, smax=smax, q_heads=nh, kv_heads=nkv, kd=kd,
                     vd=vd, **(fa_kw or {}))
    ops.gemm_fused(A, W, q, fa, epi=ops.EPI_QKV_ROPE | lf | (ops.SLOT_ROWS if slot_rows else 0), M=M,
                   **(extra or {}))
    torch.cuda.synchronize()
    for name, got, w in zip(("q", "kc", "vtc", "kd", "vd"), (q, kc, vtc, kd, vd), want):
        R.assert_all(R.exact_bf16(got.contiguous(), torch.from_numpy(w).cuda()), f"{what} {name}")
    pads_untouched(buf, M, nh * hd)


# M 1, 3: one tile per workgroup (M <= 4); M 8: the one-tile form launch_gemv_pro picks for q|k|v at M > 4; 40 x 2560:
# 1 * 20 = 20 workgroups -> 64 x 64 tiles; 264 x 2560 at H 2048: finalize_split = 2 (5 * 20 = 100 tiles <= 100)
@pytest.mark.parametrize("M,L,H,slot_rows", [(1, 1, 512, False), (3, 1, 512, False), (8, 1, 512, False),
                                             (8, 2, 512, True), (40, 20, 512, False), (40, 10, 512, True),
                                             (264, 264, 2048, False)])
def test_qkv_rope_epilogue_exact(M, L, H, slot_rows):
    """PG_EPI_QKV_ROPE at D 256, 8 query heads and one kv head, with rope_tables_exact: the reference rotates the
    exact accumulator and rounds once, as epi_qkv_rope4_core does on fp32.  GEMV (M 1, 3, 8), the tile route (M 40,
    L 20) and split + finalize (M 264, H 2048); PG_SLOT_ROWS with unequal slots once on the GEMV and once on the tile,
    one batch row's slot past the cache (not appended).  Row-major and fragment-packed W."""
    from pghip import ops
    from pghip.weights import frag_pack
    nh, nkv, hd, smax = 8, 1, 256, 320
    N = (nh + 2 * nkv) * hd
    assert (ops.finalize_split(M, N, H) == 2) == (M == 264)
    if 16 < M < 264:
        assert tile_route(M, N, 1, 0, False) == "t64x64-auto"
    p = R.exact_pair(M, N, H, seed=M + H)
    A, W = R.poisoned(cu(p.A), cu(p.W))
    for name, Wl, lf in (("row", W, 0), ("frag", frag_pack(cu(p.W)), ops.W_FRAG)):
        _qkv_case(ops, p, A, Wl, lf, M=M, L=L, nh=nh, nkv=nkv, hd=hd, smax=smax, slot_rows=slot_rows,
                  what=f"QKV M {M} L {L} H {H} {name}")


@pytest.mark.parametrize("D,nkv", [(32, 2), (256, 1)])
def test_rope_kv_write_exact(D, nkv):
    """pg_rope_kv_write on its own with the exact tables and bf16-exact integer q|k|v: q rotated in place, k into the
    cache rows, v transposed, each rounded once; the k and v columns of the input and every other cache slot are
    untouched."""
    from pghip import ops
    nh, L, B, smax = 4, 5, 2, 64
    T, nblk = B * L, nh + 2 * nkv
    g = torch.Generator().manual_seed(D)
    x64 = torch.randint(-100, 101, (T, nblk * D), generator=g).double()
    pos = torch.randint(0, 48, (T,), generator=g).to(torch.int32)
    cos_t, sin_t = R.rope_tables_exact(48, D, seed=D + 1)
    slots = [3 + 4 + t % L for t in range(T)]
    q, kcw, vtw, _, _ = R.qkv_rope_ref(x64, pos, cos_t, sin_t, L=L, Hq=nh, Hkv=nkv, D=D, smax=smax, slots=slots,
                                       fill=SENT, round_input=True)
    buf, qkv = padded(T, nblk * D, torch.bfloat16)
    qkv.copy_(x64.to(torch.bfloat16))
    kc = torch.full((B, smax, nkv * D), SENT, dtype=torch.bfloat16, device="cuda")
    vtc = torch.full((B, nkv * D, smax), SENT, dtype=torch.bfloat16, device="cuda")
    ops.rope_kv_write(qkv, cu(pos), cu(cos_t), cu(sin_t), kc, vtc, T=T, L=L, Hq=nh, Hkv=nkv, D=D, Smax=smax,
                      slot_base=3, slot_dev=torch.tensor([4], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    R.assert_all(R.exact_bf16(qkv[:, :nh * D].contiguous(), torch.from_numpy(q).cuda()), "q")
    assert torch.equal(qkv[:, nh * D:].double().cpu(), x64[:, nh * D:])
    R.assert_all(R.exact_bf16(kc, torch.from_numpy(kcw).cuda()), "kc")
    R.assert_all(R.exact_bf16(vtc, torch.from_numpy(vtw).cuda()), "vtc")
    pads_untouched(buf, T, nblk * D)


# ------------------------------------------------------------------------------------------ fp8
def _fp8_operands(p, frag=False):
    from pghip.weights import frag_pack8
    A8, W8 = R.poisoned(cu(p.A8), cu(p.W8), K_pad=16)               # (lda stays a multiple of 16 bytes)
    return A8, (frag_pack8(cu(p.W8)) if frag else W8)


# fp8 launch_tile (no auto 64 x 64): 100 x 300 and 300 x 704 -> 64 x 128 (2 * 3 and 5 * 6 workgroups); 1100 x 3712 ->
# 128 x 128; 4113 x 3856 -> 256 x 256 for F32 / F32_RES only, the 128 x 128 tile for BF16; 300 x 704 with PG_TILE_N64
# -> 64 x 64.
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M,N,flags,route", [(100, 300, 0, "t64x128"), (300, 704, 0, "t64x128"),
                                             (1100, 3712, 0, "t128x128"), (4113, 3856, 0, "g256"),
                                             (300, 704, 0x800, "t64x64-flag")])
def test_fp8_tile_routes_exact(M, N, flags, route, K):
    """ops.gemm8 on the tile routes at one and three 128-k tiles: F32 at ks 1 and a ragged ks 2, F32_RES and BF16, exact
    with power-of-two row scales."""
    from pghip import ops
    assert tile_route(M, N, 1, flags, True, fp8=True) == route
    assert tile_route(M, N, 1, flags, False, fp8=True) == ("t128x128" if route == "g256" else route)
    p = R.exact_pair_fp8(M, N, K, seed=M + K)
    A8, W8 = _fp8_operands(p)
    sa, sw, bias = cu(p.a_scale), cu(p.w_scale), cu(p.bias)
    ref = ref_dev(p)
    what = f"fp8 {route} M {M} N {N} K {K}"
    for ks in (1, 2):
        buf, part = padded(ks * M, N, torch.float32, lead=ks)
        ops.gemm8(A8, sa, W8, sw, part, epi=ops.EPI_F32 | flags, bias=bias, ksplit=ks, M=M)
        R.assert_all(R.exact_f32(part.sum(0), ref), what + f" F32 ks {ks}")
        pads_untouched(buf, ks * M, N)
    resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(K)).double().cuda()
    buf, out = padded(M, N, torch.float32)
    out.copy_(resid64.float())
    ops.gemm8(A8, sa, W8, sw, out, epi=ops.EPI_F32_RES | flags, bias=bias, M=M)
    R.assert_all(R.exact_f32(out, resid64 + ref), what + " F32_RES")
    pads_untouched(buf, M, N)
    buf, out = padded(M, N, torch.bfloat16)
    ops.gemm8(A8, sa, W8, sw, out, epi=ops.EPI_BF16 | flags, bias=bias, M=M)
    R.assert_all(R.exact_bf16(out, ref), what + " BF16")
    pads_untouched(buf, M, N)


def gemv8_form(N, K, ks, mx):
    """launch_gemv8's choice for the F32 / F32_ADD / BF16 epilogues (csrc/gemm_gemv8.hip), restated.  tiles = N / 16,
    nch = K / 128 chunks, per_z = ceil(nch / ks) a split.  The wide form (gemv8x_kernel: x once per workgroup in LDS)
    when a split's x fits (per_z * 128 <= 4096), with MX rows only at an exact 8 or 16 chunks a split, and its grid has
    >= 256 workgroups at two tiles per wave (ceil(tiles / 8) * ks) or at one (ceil(tiles / 4) * ks); its chunk count is
    a compile-time 8 or 16 when the split is exact, else the runtime loop (0).  Otherwise the K-split form
    (gemv8_kernel), chunks per wave nch / ks / 4 a compile-time 2, 4 or 8 when that division is exact, else the
    runtime loop (0)."""
    tiles, nch = N // 16, K // 128
    per_z, exact = ceil(nch, ks), nch % ks == 0
    if per_z * 128 <= 4096 and (not mx or (exact and per_z in (8, 16))):
        ct = per_z if exact and per_z in (8, 16) else 0
        if ceil(tiles, 8) * ks >= 256:
            return ("wide", 2, ct)
        if ceil(tiles, 4) * ks >= 256:
            return ("wide", 1, ct)
    cpw = nch // ks // 4 if exact and (nch // ks) % 4 == 0 else 0
    return ("ksplit", cpw if cpw in (2, 4, 8) else 0)


# form -> (N, K, ks, the kernel with a_scale rows, the kernel with MX rows in):
#   512 x 256 ks 1:     32 tiles, 2 chunks                          -> K-split, runtime loop (both)
#   1024 x 1152 ks 2:   9 chunks in splits of 5 + 4                 -> K-split, runtime loop, ragged (both)
#   4096 x 2048 ks 2:   256 tiles: 32 * 2, 64 * 2 < 256; 16 / 2 / 4 -> K-split, 2 chunks per wave (both)
#   2560 x 2048 ks 1:   160 tiles (the decode q|k|v); 16 / 4        -> K-split, 4 chunks per wave (both)
#   2048 x 16384 ks 4:  128 tiles: 16 * 4, 32 * 4 < 256; 128 / 4 / 4 -> K-split, 8 chunks per wave (both)
#   16384 x 256 ks 1:   1024 tiles: 128 < 256 <= 256, 2 chunks      -> wide, one tile per wave, runtime loop; MX rows
#                       (2 is neither 8 nor 16) -> K-split, runtime loop
#   16384 x 1024 ks 2:  128 * 2 = 256, 4 chunks a split             -> wide, two tiles, runtime loop; MX -> K-split
#   16384 x 1152 ks 2:  9 chunks in 5 + 4                           -> wide, two tiles, ragged; MX -> K-split, ragged
#   16384 x 2048 ks 1:  16 chunks                                   -> wide, one tile per wave, compile-time 16 (both:
#                       the MX wide kernel, gemv8x_kernel<..., MX>)
#   16384 x 2048 ks 2:  8 chunks a split, 128 * 2 = 256             -> wide, two tiles per wave, compile-time 8 (both)
#   2048 x 16384 ks 8:  16 chunks a split, 32 * 8 = 256 (the decode down projection) -> wide, one tile, 16 through a
#                       split (both)
FP8_GEMV = {
    "ksplit": (512, 256, 1, ("ksplit", 0), ("ksplit", 0)),
    "ksplit-ragged": (1024, 1152, 2, ("ksplit", 0), ("ksplit", 0)),
    "ksplit-cpw2": (4096, 2048, 2, ("ksplit", 2), ("ksplit", 2)),
    "ksplit-cpw4": (2560, 2048, 1, ("ksplit", 4), ("ksplit", 4)),
    "ksplit-cpw8": (2048, 16384, 4, ("ksplit", 8), ("ksplit", 8)),
    "wide1": (16384, 256, 1, ("wide", 1, 0), ("ksplit", 0)),
    "wide2": (16384, 1024, 2, ("wide", 2, 0), ("ksplit", 0)),
    "wide-ragged": (16384, 1152, 2, ("wide", 2, 0), ("ksplit", 0)),
    "wide1-ct16": (16384, 2048, 1, ("wide", 1, 16), ("wide", 1, 16)),
    "wide2-ct8": (16384, 2048, 2, ("wide", 2, 8), ("wide", 2, 8)),
    "wide1-ct16-split": (2048, 16384, 8, ("wide", 1, 16), ("wide", 1, 16)),
}


@functools.lru_cache(maxsize=None)
def _fp8_gemv_pair(form):
    """One 32-row pair per form, shared by the row counts and by the a_scale and MX cases (read-only): the operands and
    the float64 W on the device, the CPU copies of the large matrices dropped."""
    from pghip.weights import frag_pack8
    N, K = FP8_GEMV[form][:2]
    p = R.exact_pair_fp8(32, N, K, seed=N + K, mx=True)
    A8, _ = R.poisoned(cu(p.A8), cu(p.W8[:16]), K_pad=16)
    p.A8d, p.W8f, p.W64d = A8, frag_pack8(cu(p.W8)), cu(p.W64)
    p.A64_rows = p.Aq64 * p.a_scale.double()[:, None]            # the product with a_scale rows; p.A64 is the MX one
    p.W8 = p.W64 = p.Wq64 = None
    return p


@pytest.mark.parametrize("M", [9, 17, 32])
@pytest.mark.parametrize("form", list(FP8_GEMV))
def test_fp8_gemv_exact(form, M):
    """The fp8 weight-streaming GEMV (fragment-packed e4m3 W) at 9, 17 and 32 rows (one and two 16-row x tiles; at
    M > 16 and a small grid the row-split form), on every kernel form of the table above -- the K-split kernel with the
    runtime chunk loop and with 2, 4 and 8 chunks per wave, the wide kernel with the runtime loop and with a
    compile-time 8 and 16 chunks, plain and through a K split: F32 slabs, F32_ADD onto an integer residual and BF16
    (ks 1) are exact.
    MX rows in (E8M0 block scales 2^-2 .. 2^2 applied inside the MFMA, a_scale not read) are exact on the kernel the
    table's last column names: the MX wide kernel only at 8 or 16 chunks a split, the MX K-split kernel elsewhere."""
    from pghip import ops
    N, K, ks, form_rows, form_mx = FP8_GEMV[form]
    assert gemv8_form(N, K, ks, False) == form_rows and gemv8_form(N, K, ks, True) == form_mx
    p = _fp8_gemv_pair(form)
    A8, W8f = p.A8d[:M], p.W8f
    sw, bias = cu(p.w_scale), cu(p.bias)
    for mx in (False, True):
        sa = None if mx else cu(p.a_scale)
        kw = dict(mx_in=cu(R.mx_frag_order(p.mx[:M]))) if mx else {}
        ref = ((p.A64 if mx else p.A64_rows)[:M].cuda() @ p.W64d.t()) + cu(p.bias64)
        what = f"fp8 gemv {form} M {M} mx {mx}"
        buf, part = padded(ks * M, N, torch.float32, lead=ks)
        ops.gemm8(A8, sa, W8f, sw, part, epi=ops.EPI_F32, bias=bias, ksplit=ks, frag=True, M=M, **kw)
        R.assert_all(R.exact_f32(part.sum(0), ref), what + " F32")
        pads_untouched(buf, ks * M, N)
        if mx:
            continue
        resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(K)).double().cuda()
        buf, out = padded(M, N, torch.float32)
        out.copy_(resid64.float())
        ops.gemm8(A8, sa, W8f, sw, out, epi=ops.EPI_F32_ADD, bias=bias, ksplit=ks, frag=True, M=M)
        R.assert_all(R.exact_f32(out, resid64 + ref), what + " F32_ADD")
        pads_untouched(buf, M, N)
        if ks == 1:
            buf, out = padded(M, N, torch.bfloat16)
            ops.gemm8(A8, sa, W8f, sw, out, epi=ops.EPI_BF16, bias=bias, frag=True, M=M)
            R.assert_all(R.exact_bf16(out, ref), what + " BF16")
            pads_untouched(buf, M, N)


@pytest.mark.parametrize("M,N,K,ks", [(300, 384, 384, 1), (300, 384, 384, 2), (1100, 3712, 128, 1)])
def test_fp8_mx_rows_prefill_tile_exact(M, N, K, ks):
    """MX rows into the prefill tile GEMM (the 128 x 128 fp8 tile with per-lane block scales, natural scale order
    [M][K/32]): F32 slabs and F32_RES exact."""
    from pghip import ops
    assert tile_route(M, N, ks, 0, True, fp8=True, mx=True) == "t128x128-mx"
    p = R.exact_pair_fp8(M, N, K, seed=M + K + 1, mx=True)
    A8, W8 = _fp8_operands(p)
    ref = ref_dev(p)
    buf, part = padded(ks * M, N, torch.float32, lead=ks)
    ops.gemm8(A8, None, W8, cu(p.w_scale), part, epi=ops.EPI_F32, bias=cu(p.bias), ksplit=ks, M=M, mx_in=cu(p.mx))
    R.assert_all(R.exact_f32(part.sum(0), ref), f"mx tile M {M} ks {ks}")
    pads_untouched(buf, ks * M, N)
    if ks == 1:
        resid64 = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(K)).double().cuda()
        buf, out = padded(M, N, torch.float32)
        out.copy_(resid64.float())
        ops.gemm8(A8, None, W8, cu(p.w_scale), out, epi=ops.EPI_F32_RES, bias=cu(p.bias), M=M, mx_in=cu(p.mx))
        R.assert_all(R.exact_f32(out, resid64 + ref), f"mx tile M {M} F32_RES")
        pads_untouched(buf, M, N)


@pytest.mark.parametrize("M,N,K,frag", [(300, 704, 128, False), (1100, 3712, 128, False), (9, 512, 256, True),
                                        (32, 512, 256, True)])
def test_fp8_gelu_mul_within_delta(M, N, K, frag):
    """gelu(gate) * up on the fp8 tile (64 x 128 and 128 x 128) and the fp8 GEMV."""
    from pghip import ops
    p = R.gelu_pair_fp8(M, N, K, seed=M + N)
    A8, W8 = _fp8_operands(p, frag=frag)
    buf, out = padded(M, N // 2, torch.bfloat16)
    ops.gemm8(A8, cu(p.a_scale), W8, cu(p.w_scale), out, epi=ops.EPI_BF16_GELU_MUL, frag=frag, M=M)
    R.assert_all(R.within_bf16(out, R.gelu_mul64(ref_dev(p)), R.GELU_DELTA), f"fp8 GELU_MUL M {M} frag {frag}")
    pads_untouched(buf, M, N // 2)
