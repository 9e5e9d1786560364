"""The lossless 13-bit weight pack (include/pghip.h PG_W_FRAG13) on the host: weights.frag13_pack / frag13_unpack are
torch ops that run on CPU tensors, so the layout's round trip, its fit rule and its size are checked without a device."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

from oracle import synth
from pghip import weights

BLOCK = 3328


def _bits(w: torch.Tensor) -> torch.Tensor:
    return w.contiguous().view(torch.int16)


def _bf16_from_fields(sign, exp, mant) -> torch.Tensor:
    v = (sign.to(torch.int32) << 15) | (exp.to(torch.int32) << 7) | mant.to(torch.int32)
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(torch.bfloat16)


def _random_fields(shape, lo: int, hi: int, seed: int) -> torch.Tensor:
    """bf16 values with random signs and mantissas and exponent fields uniform in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    return _bf16_from_fields(torch.randint(0, 2, shape, generator=g), torch.randint(lo, hi + 1, shape, generator=g),
                             torch.randint(0, 128, shape, generator=g))


def _roundtrip(w: torch.Tensor) -> torch.Tensor:
    p = weights.frag13_pack(w)
    assert p is not None and p.dtype == torch.uint8 and p.dim() == 1
    N, K = w.shape
    assert p.numel() == (N // 16) * (K // 128) * BLOCK + (N // 16) * (K // 128) * 2 == weights.frag13_size(N, K)
    back = weights.frag13_unpack(p, N, K)
    assert back.dtype == torch.bfloat16 and torch.equal(_bits(back), _bits(w))
    return p


def test_synthetic_matrix_roundtrip():
    # (the smallest K with a whole group of eight 64-k chunks is 512: a block pairs chunks c and c + 4 of a group)
    w = torch.from_numpy(synth.generate("language_model.model.layers.0.mlp.gate_proj.weight", (64, 512))).bfloat16()
    _roundtrip(w)


def test_normal_matrix_roundtrip():
    g = torch.Generator().manual_seed(13)
    w = (torch.randn(48, 1024, generator=g) * 0.02).bfloat16()
    _roundtrip(w)


def test_all_zero_block():
    w = _random_fields((32, 512), 110, 126, 1)
    w[:16, :] = 0.0                                   # tile 0: every block all zeros
    p = _roundtrip(w)
    tab = p[(32 // 16) * (512 // 128) * BLOCK:].view(-1, 2)
    assert tab[:4, 0].tolist() == [1] * 4 and tab[:4, 1].tolist() == [1] * 4     # base 1, zero flag set
    assert tab[4:, 1].tolist() == [0] * 4


def test_zeros_and_denormals_among_normals():
    w = _random_fields((16, 512), 100, 127, 2)
    b = _bits(w).clone()
    b[0, 0], b[3, 77], b[15, 511] = 0, -32768, 0x0001               # +0, -0, smallest denormal
    b[7, 130], b[9, 300] = 0x007F, np.int16(-32768 + 0x40)          # largest denormal, a negative denormal
    _roundtrip(b.view(torch.bfloat16))


def test_block_spanning_exactly_31_codes_fits_and_32_does_not():
    w = _random_fields((16, 512), 120, 120, 3)
    b = _bits(w).clone()
    b[2, 5] = (90 << 7) | 0x11                         # block (0, 0): fields 90 .. 120 = 31 codes
    b[4, 6] = (120 << 7) | 0x22
    w31 = b.view(torch.bfloat16)
    _roundtrip(w31)
    b[2, 5] = (89 << 7) | 0x11                         # 89 .. 120 = 32 codes
    assert weights.frag13_pack(b.view(torch.bfloat16)) is None


def test_inf_nan_in_a_narrow_block():
    w = _random_fields((16, 512), 230, 254, 4)
    b = _bits(w).clone()
    b[1, 1] = 0x7F80                                   # +inf
    b[1, 2] = np.int16(-128)                           # 0xFF80 -inf
    b[5, 200] = 0x7FC1                                 # a NaN with payload
    _roundtrip(b.view(torch.bfloat16))


def test_shapes_without_whole_blocks_are_not_packed():
    w = _random_fields((64, 256), 110, 126, 5)
    assert weights.frag13_pack(w) is None              # K 256: no whole group of eight chunks
    assert weights.frag13_pack(_random_fields((24, 512), 110, 126, 6)) is None
    with pytest.raises(ValueError):
        weights.frag13_unpack(torch.zeros(10, dtype=torch.uint8), 16, 512)


def check_boundary_rejections():
    """pg_gemm_fused with PG_W_FRAG13 returns hipErrorInvalidValue for every argument the layout or its instantiated
    forms do not cover -- before any HIP call, so no device is needed (the pointers are never dereferenced)."""
    import ctypes as C
    from pghip import _lib, ops
    lib = _lib.load()
    INVALID = 1                                           # hipErrorInvalidValue
    p = 0x1000                                            # non-null, 16-byte aligned, never dereferenced

    def call(epi=ops.EPI_FX_ADD, pro=0, W=p, M=1, N=48, K=2048, ks=1, ldw=None, extra=0, **fields):
        fa = ops.fused_args(pro_mode=pro, **fields)
        return lib.pg_gemm_fused(p, K, W, K if ldw is None else ldw, None, p, N, M, N, K,
                                 epi | ops.W_FRAG13 | extra, ks, C.byref(fa), None)

    assert call(W=None) == INVALID
    assert call(W=p + 8) == INVALID                       # misaligned pack
    assert call(N=40) == INVALID                          # N % 16
    assert call(K=2048 + 64) == INVALID                   # K % 128
    assert call(K=1024 + 128) == INVALID                  # chunks per split % 8
    assert call(ks=8) == INVALID                          # 2048 / 64 / 8 = 4 chunks per split
    assert call(ks=0) == INVALID
    assert call(M=5) == INVALID and call(M=16) == INVALID and call(M=0) == INVALID
    assert call(ldw=4096) == INVALID
    assert call(extra=ops.W_FRAG) == INVALID              # one layout flag at a time
    assert call(extra=ops.EPI_FP8) == INVALID
    # forms that are not instantiated
    assert call(epi=ops.EPI_BF16) == INVALID
    assert call(epi=ops.EPI_F32) == INVALID               # plain x into fp32 slabs
    assert call(epi=ops.EPI_F32_ADD) == INVALID
    assert call(epi=ops.EPI_BF16_GELU_MUL, N=96) == INVALID               # gate/up without the RMSNorm prologue
    assert call(epi=ops.EPI_FX_ADD, pro=1, resid_in=p, norm_w=p) == INVALID
    assert call(epi=ops.EPI_F32_FIN, pro=2) == INVALID


def test_boundary_rejections():
    check_boundary_rejections()


def test_budget_is_at_most_13_1_bits_per_weight():
    assert weights.frag13_size(2048, 16384) * 8 / (2048 * 16384) <= 13.1
