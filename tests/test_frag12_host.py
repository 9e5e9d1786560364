"""The 12-bit form of the exponent-coded weight pack (include/pghip.h PG_W_FRAG12) on the host: weights.frag12_pack /
frag12_unpack are torch ops that run on CPU tensors, so the round trip, the narrow / wide rule, the heap and the size are
checked without a device.  The block geometry is restated here (rows 16t .. 16t + 15 x the 64-k chunks c = 8i + w and
c + 4), not taken from the packer."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

from oracle import synth
from pghip import weights
from test_frag13_host import _bits, _random_fields

N, K = 64, 512          # the smallest shape with whole blocks (K % 512), four tiles x four blocks


def block_index(t: int, b: int):
    """(rows, columns) of block (t, b) of a row-major matrix."""
    c = 8 * (b // 4) + b % 4
    cols = torch.cat([torch.arange(64 * c, 64 * c + 64), torch.arange(64 * (c + 4), 64 * (c + 4) + 64)])
    return torch.arange(16 * t, 16 * t + 16)[:, None], cols[None, :]


def field(e: int, m: int = 0x15) -> int:
    return (e << 7) | m


def hand_built():
    """The 64 x 512 matrix of fields 110 .. 120 (narrow) with hand-made blocks, and {(t, b): (wide, zflag)} for them."""
    b = _bits(_random_fields((N, K), 110, 120, 12)).clone()
    want = {}

    def put(t, blk, items, wide, zflag):
        r, c = block_index(t, blk)
        for (i, j), v in items.items():
            b[r[i, 0], c[0, j]] = v
        want[(t, blk)] = (wide, zflag)

    put(0, 0, {(0, 0): field(105), (3, 70): field(120)}, 0, 0)           # span exactly 15: narrow
    put(0, 1, {(0, 0): field(104), (3, 70): field(120)}, 1, 0)           # span exactly 16: wide
    put(0, 2, {(5, 9): 0}, 1, 1)                                         # one zero weight
    r, c = block_index(0, 3)
    b[r, c] = 0                                                          # an all-zero block
    want[(0, 3)] = (1, 1)
    put(1, 0, {(15, 127): field(130)}, 1, 0)                             # wide only through its last element (row 15,
    put(1, 1, {(15, 127): -32768}, 1, 1)                                 # k 64(c + 4) + 63): a far field, and a -0
    put(1, 2, {(2, 5): field(90), (4, 6): field(120)}, 1, 0)             # span 30: 31 codes, the widest that packs
    put(2, 3, {(0, 0): field(110), (1, 1): field(125)}, 0, 0)            # narrow at another base
    return b.view(torch.bfloat16), want


def roundtrip(w: torch.Tensor):
    p = weights.frag12_pack(w)
    assert p is not None and p.dtype == torch.uint8 and p.dim() == 1
    n, k = w.shape
    bias, zflag, wide, line, nlines = weights.frag12_table(p, n, k)
    assert p.numel() == weights.frag12_size(n, k, int(wide.sum()))
    back = weights.frag12_unpack(p, n, k)
    assert back.dtype == torch.bfloat16 and torch.equal(_bits(back), _bits(w))
    return p, bias, zflag, wide, line, nlines


def test_hand_built_blocks_roundtrip_flags_and_heap():
    w, want = hand_built()
    p, bias, zflag, wide, line, nlines = roundtrip(w)
    for t in range(N // 16):
        for b in range(K // 128):
            exp_wide, exp_z = want.get((t, b), (0, 0))
            assert (int(wide[t, b]), int(zflag[t, b])) == (exp_wide, exp_z), (t, b)
    # the heap: the shared zero line, then exactly the wide blocks in block order
    H = sum(v[0] for v in want.values())
    assert H == 6 and nlines == H + 1
    assert line[wide == 0].abs().sum() == 0
    assert line[wide == 1].tolist() == list(range(1, H + 1))
    nblk = (N // 16) * (K // 128)
    heap = p[nblk * 3072 + 256:]                         # 16 blocks' table: 64 bytes, padded to one 256-B line
    assert heap.numel() == 256 * (H + 1) and not bool(heap[:256].any())
    assert p.numel() == nblk * 3072 + 256 + 256 * (H + 1)
    # biases: a narrow block's smallest field; a wide block's base - 1; 0 for the all-zero block
    assert int(bias[0, 0]) == 105 and int(bias[0, 1]) == 103 and int(bias[0, 3]) == 0 and int(bias[1, 2]) == 89
    assert int(bias[2, 3]) == 110
    # the fifth plane of the block that is wide through its last element alone: one bit, pair 15's o = 1, lane 63
    l10 = heap[256 * int(line[1, 0]):][:256].view(64, 4)
    assert l10[:63].sum() == 0 and l10[63].tolist() == [0, 0, 0, 0x80]


def test_span_32_does_not_pack():
    w, _ = hand_built()
    b = _bits(w).clone()
    r, c = block_index(1, 2)
    b[r[2, 0], c[0, 5]] = field(89)                      # 89 .. 120 in one block
    assert weights.frag12_pack(b.view(torch.bfloat16)) is None
    assert weights.frag13_pack(b.view(torch.bfloat16)) is None      # the same rule as the 13-bit form


def test_synthetic_and_normal_matrices_roundtrip():
    w = torch.from_numpy(synth.generate("language_model.model.layers.0.mlp.gate_proj.weight", (N, K))).bfloat16()
    roundtrip(w)
    g = torch.Generator().manual_seed(13)
    roundtrip((torch.randn(48, 1024, generator=g) * 0.02).bfloat16())


def test_inf_nan_and_denormals():
    b = _bits(_random_fields((16, 512), 241, 254, 4)).clone()
    b[1, 1], b[1, 2], b[5, 200] = 0x7F80, -128, 0x7FC1           # +inf, -inf, a NaN with payload (field 255: span 14)
    _, _, _, wide, _, _ = roundtrip(b.view(torch.bfloat16))
    assert int(wide.sum()) == 0
    b[7, 130] = 0x007F                                           # the largest denormal: field 0
    b2 = _bits(_random_fields((16, 512), 1, 14, 5)).clone()
    b2[0, 0] = 0x0001
    for m in (b, b2):
        assert int(roundtrip(m.view(torch.bfloat16))[3].sum()) == 1


def test_narrow_share_of_a_synthetic_matrix():
    """The packer's narrow share of a 256 x 2048 synthetic gate_proj against the rule applied to the matrix directly."""
    n, k = 256, 2048
    w = torch.from_numpy(synth.generate("language_model.model.layers.0.mlp.gate_proj.weight", (n, k))).bfloat16()
    p, _, _, wide, _, _ = roundtrip(w)
    E = (_bits(w).to(torch.int32) >> 7) & 0xFF
    narrow = 0
    for t in range(n // 16):
        for b in range(k // 128):
            e = E[block_index(t, b)]
            narrow += int(e.min() > 0 and e.max() - e.min() <= 15)
    nblk = (n // 16) * (k // 128)
    share = 1.0 - float(wide.sum()) / nblk
    print(f"narrow share {share:.4f} (direct count {narrow / nblk:.4f}), "
          f"{p.numel() * 8 / (n * k):.3f} bits per weight")
    assert abs(share - narrow / nblk) <= 0.01
    # 12 bits, the table word, one more bit per weight of a wide block; the shared line and the table's padding: < 0.01
    assert p.numel() * 8 / (n * k) <= 12.0 + 32 / 2048 + (1 - share) + 0.01


def test_shapes_without_whole_blocks_are_not_packed():
    assert weights.frag12_pack(_random_fields((64, 256), 110, 126, 5)) is None
    assert weights.frag12_pack(_random_fields((24, 512), 110, 126, 6)) is None
    with pytest.raises(ValueError):
        weights.frag12_unpack(torch.zeros(10, dtype=torch.uint8), 16, 512)


def check_boundary_rejections():
    """pg_gemm_fused with PG_W_FRAG13 | PG_W_FRAG12 returns hipErrorInvalidValue where the 13-bit flag does, before any
    HIP call (the pointers are never dereferenced) -- and for PG_W_FRAG12 without PG_W_FRAG13."""
    import ctypes as C
    from pghip import _lib, ops
    lib = _lib.load()
    INVALID = 1                                           # hipErrorInvalidValue
    p = 0x1000                                            # non-null, 16-byte aligned, never dereferenced

    def call(epi=ops.EPI_FX_ADD, pro=0, W=p, M=1, N=48, K=2048, ks=1, ldw=None, extra=0,
             flag=ops.W_FRAG13 | ops.W_FRAG12, **fields):
        fa = ops.fused_args(pro_mode=pro, **fields)
        return lib.pg_gemm_fused(p, K, W, K if ldw is None else ldw, None, p, N, M, N, K, epi | flag | extra, ks,
                                 C.byref(fa), None)

    assert call(flag=ops.W_FRAG12) == INVALID             # the modifier alone
    assert call(flag=ops.W_FRAG12 | ops.W_FRAG) == INVALID
    assert call(W=None) == INVALID
    assert call(W=p + 8) == INVALID                       # misaligned pack
    assert call(N=40) == INVALID                          # N % 16
    assert call(K=2048 + 64) == INVALID                   # K % 128
    assert call(K=1024 + 128) == INVALID                  # K not in whole blocks per wave
    assert call(ks=8) == INVALID                          # 2048 / 64 / 8 = 4 chunks per split
    assert call(ks=0) == INVALID
    assert call(M=5) == INVALID and call(M=16) == INVALID and call(M=0) == INVALID      # wrong M
    assert call(ldw=4096) == INVALID
    assert call(extra=ops.W_FRAG) == INVALID
    assert call(extra=ops.EPI_FP8) == INVALID             # with fp8
    assert call(epi=ops.EPI_BF16) == INVALID              # forms that are not instantiated
    assert call(epi=ops.EPI_F32_ADD) == INVALID
    assert call(epi=ops.EPI_BF16_GELU_MUL, N=96) == INVALID
    assert call(epi=ops.EPI_F32_FIN, pro=2) == INVALID


def test_boundary_rejections():
    check_boundary_rejections()


def test_ops_checks_the_pack_length():
    from pghip import ops
    nblk = 3 * 16
    assert ops._packed_len_ok(weights.frag12_size(48, 2048, 0), nblk, True)
    assert ops._packed_len_ok(weights.frag12_size(48, 2048, nblk), nblk, True)
    assert not ops._packed_len_ok(weights.frag12_size(48, 2048, nblk + 1), nblk, True)
    assert not ops._packed_len_ok(weights.frag12_size(48, 2048, 0) - 256, nblk, True)
    assert not ops._packed_len_ok(weights.frag13_size(48, 2048), nblk, True)
    assert ops._packed_len_ok(weights.frag13_size(48, 2048), nblk, False)
