"""The two-part first fill of the 12-bit GEMV forms that read x straight from memory (csrc/gemm_gemv.hip
PG_GEMV_W12_SPLIT): down (PG_EPI_FX_ADD, plain rows), the finalising down (PG_EPI_F32_FIN) and the lm_head
(PG_EPI_F32 behind PRO_X_RSTD), each launched with the bf16 fragment pack and with the 12-bit pack of the same matrix:
torch.equal outputs.  The matrices (tests/test_frag12_fill_host.py) hold one wide block at each position of a wave's
strip in turn -- the first fill's first, middle and last block and, in the lm_head, the first refill -- a zero-coded wide
block at either end, one wide block per tile, and every block wide.  K = 2048 is the straight-line form of 8 chunks per
wave (4 with a K split of two), K = 512 the runtime loop."""
import functools

import pytest
import torch

from test_frag12_fill_host import kinds_for, packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def weights_of(kind: str, N: int, K: int):
    """(fragment pack, 12-bit pack) on the device, built and host-checked once per matrix."""
    from pghip.weights import frag_pack
    w, p12 = packed(kind, N, K)
    return frag_pack(w.cuda()), p12.cuda()


def both(launch, kind, N, K):
    from pghip import ops
    wf, w12 = weights_of(kind, N, K)
    want = launch(wf, ops.W_FRAG, {})
    got = launch(w12, ops.W_FRAG13 | ops.W_FRAG12, dict(N=N, K=K))
    torch.cuda.synchronize()
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (i, kind, N, K)
    return want


PRO0 = [(48, 2048, 1, k) for k in kinds_for(2048)] + [(48, 2048, 2, k) for k in kinds_for(2048)] + \
       [(48, 512, 1, k) for k in kinds_for(512)]
LM = [(80, K, k) for K in (2048, 512) for k in kinds_for(K)]


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K,ks,kind", PRO0)
def test_fx_add_plain_rows(M, N, K, ks, kind):
    """PG_EPI_FX_ADD, pro_mode 0 (down): the fixed-point accumulator after the launch."""
    from pghip import ops
    x = rnd(M, K, scale=0.5, seed=21)
    bias = rnd(N, seed=22, dtype=torch.float32)

    def launch(W, flag, nk):
        acc = torch.full((M, N), 12345, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.gemm_fused(x, W, acc, ops.fused_args(status=st), epi=ops.EPI_FX_ADD | flag, M=M, ksplit=ks, bias=bias, **nk)
        return acc, st

    acc, st = both(launch, kind, N, K)
    assert int(st) == 0 and bool((acc != 12345).any())


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K,ks,kind", PRO0)
def test_f32_fin_last_down(M, N, K, ks, kind):
    """PG_EPI_F32_FIN, pro_mode 0 (the last layer's down): finalised residual, x', sums of squares, cleared tickets and
    the cleared fixed-point accumulator."""
    from pghip import ops
    tiles = N // 16
    x = rnd(M, K, scale=0.5, seed=41)
    nw = rnd(N, scale=0.1, seed=42, dtype=torch.float32)
    fx0 = (rnd(M, N, seed=43, dtype=torch.float32).double() * 2.0 ** 32).round().to(torch.int64)

    def launch(W, flag, nk):
        part = torch.zeros(ks, M, N, device="cuda")
        cnt = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        res = rnd(M, N, seed=44, dtype=torch.float32)
        ss = torch.zeros(M, tiles, device="cuda")
        xq = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        fx = fx0.clone()
        fa = ops.fused_args(fin_cnt=cnt, fin_resid=res, ss_out=ss, ss_ld=tiles, fin_x=xq, norm_w=nw, fx=fx)
        ops.gemm_fused(x, W, part, fa, epi=ops.EPI_F32_FIN | flag, M=M, ksplit=ks, **nk)
        return res, xq, ss, cnt, fx

    res, xq, ss, cnt, fx = both(launch, kind, N, K)
    assert not bool(cnt.any()) and not bool(fx.any()) and bool(ss.abs().sum() > 0)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K,kind", LM)
def test_lm_head_rstd_prologue(M, N, K, kind):
    """PG_EPI_F32, pro_mode 4, two tiles per workgroup (N = 80: the last workgroup's second tile is clamped)."""
    from pghip import ops
    x = rnd(M, K, seed=51)
    bias = rnd(N, seed=52, dtype=torch.float32)
    n_ss = 128
    ss_in = rnd(M, n_ss, seed=53, dtype=torch.float32).abs()

    def launch(W, flag, nk):
        out = torch.zeros(M, N, device="cuda")
        fa = ops.fused_args(pro_mode=ops.PRO_X_RSTD, ss_in=ss_in, ss_ld=n_ss, ss_n=n_ss, eps=1e-6)
        ops.gemm_fused(x, W, out, fa, epi=ops.EPI_F32 | flag, M=M, bias=bias, **nk)
        return (out,)

    assert bool(both(launch, kind, N, K)[0].abs().sum() > 0)
