"""The matrices of tests/test_frag12_fill_gpu.py, built and checked without a device.

The GEMV forms that read x straight from memory (down, the finalising down, the lm_head) issue their weight ring's
first fill in two parts (csrc/gemm_gemv.hip PG_GEMV_W12_SPLIT), so where a wide block sits in a wave's strip decides
which loads its decode waits for.  `fill_matrix` plants wide blocks at chosen strip positions of an otherwise narrow
matrix: block (t, 4 i + w) is the i-th block of wave w's strip of tile t (i counts over the whole K, so with a K split of
two the second split starts at i = K / 1024).  One tiny-magnitude weight makes a block wide; one zero makes it wide with
a code 0 (the table word's zero flag)."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

from pghip import weights
from test_frag12_host import block_index, field
from test_frag13_host import _bits, _random_fields

TINY, ZERO = "tiny", "zero"


def fill_matrix(N: int, K: int, plant, seed: int = 0):
    """(bf16 matrix, expected wide mask, expected zero-flag mask): fields 112 .. 124 everywhere (every block narrow), then
    for each (t, i, w, what) of `plant` one weight of block (t, 4 i + w) replaced -- TINY: field 96 (span >= 16 against
    the block's other 2047 weights), ZERO: +0."""
    T, nb = N // 16, K // 128
    b = _bits(_random_fields((N, K), 112, 124, 1000 + N + K + seed)).clone()
    wide = torch.zeros(T, nb, dtype=torch.bool)
    zflag = torch.zeros(T, nb, dtype=torch.bool)
    for n, (t, i, w, what) in enumerate(plant):
        blk = 4 * i + w
        assert 0 <= t < T and 0 <= w < 4 and 0 <= blk < nb and not wide[t, blk]
        r, c = block_index(t, blk)
        # (a different element each time: rows and both 64-k chunks of the block get their turn)
        b[r[(5 * n + 3) % 16, 0], c[0, (37 * n + 70) % 128]] = field(96) if what == TINY else 0
        wide[t, blk] = True
        zflag[t, blk] = what == ZERO
    return b.view(torch.bfloat16), wide, zflag


def plants(kind: str, N: int, K: int):
    """The plant list of a named matrix.  pos<i>: ONE wide block in the matrix, the i-th of wave 2's strip of tile 1;
    zero<i>: the same block, wide through a zero; each: every tile's wave t % 4 holds one wide block, at position
    t % (K / 512); all: every block wide, every third one through a zero."""
    T, n_i = N // 16, K // 512
    if kind.startswith("pos"):
        return [(1, int(kind[3:]), 2, TINY)]
    if kind.startswith("zero"):
        return [(1, int(kind[4:]), 2, ZERO)]
    if kind == "each":
        return [(t, t % n_i, t % 4, TINY) for t in range(T)]
    if kind == "all":
        return [(t, i, w, ZERO if (t + i + w) % 3 == 0 else TINY) for t in range(T) for i in range(n_i) for w in range(4)]
    raise ValueError(kind)


def kinds_for(K: int):
    """Every strip position of the shape in turn (K = 2048: the four blocks of a wave's strip -- in the down forms all
    four are the first fill, first / middle / middle / last; in the lm_head three are and the fourth is the first refill),
    a zero-coded wide block at the first and at the last position, one wide block per tile, every block wide."""
    n_i = K // 512
    return tuple(f"pos{i}" for i in range(n_i)) + tuple(sorted({"zero0", f"zero{n_i - 1}"})) + ("each", "all")


def packed(kind: str, N: int, K: int):
    """(row-major matrix, its 12-bit pack), the pack's table checked against the plant list."""
    w, wide, zflag = fill_matrix(N, K, plants(kind, N, K))
    p = weights.frag12_pack(w)
    assert p is not None, (kind, N, K)
    _, z, wd, line, nlines = weights.frag12_table(p, N, K)
    assert torch.equal(wd.bool(), wide), (kind, N, K)
    assert torch.equal(z.bool(), zflag), (kind, N, K)
    assert nlines == int(wide.sum()) + 1 and p.numel() == weights.frag12_size(N, K, int(wide.sum()))
    return w, p


SHAPES = [(48, 2048), (48, 512), (80, 2048), (80, 512)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_wide_blocks_are_exactly_the_planted_ones(N, K):
    n_i = K // 512
    assert kinds_for(K)[:n_i] == tuple(f"pos{i}" for i in range(n_i))
    for kind in kinds_for(K):
        w, p = packed(kind, N, K)
        _, zflag, wide, line, _ = weights.frag12_table(p, N, K)
        want = plants(kind, N, K)
        assert int(wide.sum()) == len(want)
        if kind.startswith(("pos", "zero")):
            (t, i, wv, what), = want
            assert wide.nonzero().tolist() == [[t, 4 * i + wv]] and int(line[t, 4 * i + wv]) == 1
            assert int(zflag.sum()) == (what == ZERO)
        elif kind == "each":
            assert wide.sum(1).tolist() == [1] * (N // 16) and int(zflag.sum()) == 0
        else:
            assert bool(wide.all()) and 0 < int(zflag.sum()) < wide.numel()
        back = weights.frag12_unpack(p, N, K)
        assert torch.equal(_bits(back), _bits(w)), (kind, N, K)


def test_a_planted_weight_alone_makes_its_block_wide():
    """The unplanted matrix is narrow throughout, so each wide block above is the plant's doing."""
    for N, K in SHAPES:
        w, wide, zflag = fill_matrix(N, K, [])
        assert not bool(wide.any()) and not bool(zflag.any())
        _, z, wd, _, nlines = weights.frag12_table(weights.frag12_pack(w), N, K)
        assert int(wd.sum()) == 0 and int(z.sum()) == 0 and nlines == 1


def test_positions_cover_the_first_fill_and_the_first_refill():
    """K = 2048: four blocks per wave and tile.  The down forms hold four blocks in flight (all of the strip is the first
    fill), the lm_head three (positions 0 .. 2 are the fill's first, middle and last block, position 3 the first
    refill); with a K split of two, positions 2 and 3 are the second split's first and last block."""
    assert kinds_for(2048) == ("pos0", "pos1", "pos2", "pos3", "zero0", "zero3", "each", "all")
    assert kinds_for(512) == ("pos0", "zero0", "each", "all")
    for i in range(4):
        (t, pi, wv, what), = plants(f"pos{i}", 48, 2048)
        assert (t, pi, wv, what) == (1, i, 2, TINY)
