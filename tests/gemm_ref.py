"""Exact-arithmetic inputs, float64 references and per-element checkers for the GEMM tests
(test_gemm_ref_host.py on the CPU, test_gemm_exact_gpu.py on the device).  No device dependency.

The idea: with small-integer operands scaled by powers of two, every product and every partial sum of a GEMM, in any
order, is exactly representable in fp32 (EXACT_SUM bounds sum |a||w| of every output).  The float64 product is then
the one right answer for every tile shape, K split, weight pack and accumulation order: an fp32 output must equal it
bit for bit, a bf16 output must be its round-to-nearest-even rounding bit for bit.  Epilogues with transcendental
arithmetic (tanh-GELU) are checked per element against float64 to GELU_DELTA, far below one bf16 step.

GELU_DELTA = 2^-12, from gelu_tanh in csrc/common.h, x * rcp(1 + exp2(-2.88539 u)), u = 0.79788 (x + 0.044715 x^3):
u carries 4 roundings; at |x| = 8 the exp2 argument reaches about 71 in magnitude, so its absolute error is at most
about 2.5e-5 and the relative error of the power about 2^-15.8; v_exp_f32, v_rcp_f32 and the final multiply add about
2^-22.  The total is below 2^-15: 2^-12 leaves 8x margin and is still 8x finer than the bf16 half step 2^-9.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

EXACT_SUM = 2 ** 20          # sum |a||w| of every output: any accumulator >= 21 bits wide is exact, in any order
GELU_DELTA = 2.0 ** -12
GELU_MAX = 8.0               # |pre-activation| bound of gelu_pair (beyond ~10 the kernel's exp2 overflows to its limit)
FP8_VALUES = (0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0)      # magnitudes whose e4m3 encodings exact_pair_fp8 draws
ROPE_ENTRIES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.5, 0.5), (0.5, -0.5))
NORM_C = (0.5, 1.0, 2.0, 4.0)                          # |v| of a norm_rows_exact row
NORM_W1 = (0.5, 1.0, 1.5, 2.0)                         # 1 + norm_w


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()


def default_amp(K: int) -> int:
    """The largest power of two <= 8 with K * amp * amp <= EXACT_SUM."""
    amp = 8
    while amp > 1 and K * amp * amp > EXACT_SUM:
        amp //= 2
    if K * amp * amp > EXACT_SUM:
        raise ValueError(f"K = {K} has no exact amplitude")
    return amp


# ---------------------------------------------------------------------------------------------- builders
def exact_pair(M, N, K, seed, amp=None, w_shift=True, w_exp=0, bias_step=0.5, bias_max=64.0, w_nonzero=False):
    """A [M][K], W [N][K] bf16 and bias [N] fp32 with the float64 matrices beside them.  A and W are integers in
    [-amp, amp] (amp: default_amp(K)); with w_shift row n of W is multiplied by 2^-(n % 4), so outputs are not all
    integers and exponents differ between rows; w_exp scales every row of W by 2^w_exp on top.  Bias: multiples of
    bias_step with |bias| <= bias_max.  w_nonzero: zeros in W become ones (weights whose exponent-coded blocks
    hold no zero).  sum |a||w| <= EXACT_SUM before the row scales (asserted)."""
    amp = default_amp(K) if amp is None else int(amp)
    assert amp >= 1 and amp & (amp - 1) == 0 and amp <= 8 and K * amp * amp <= EXACT_SUM, (K, amp)
    g = _gen(seed)
    A64 = _ints(g, (M, K), -amp, amp)
    Wi = _ints(g, (N, K), -amp, amp)            # (sum |a||w| <= K * amp^2 <= EXACT_SUM for every output)
    if w_nonzero:
        Wi[Wi == 0] = 1.0
    rs = torch.full((N,), 2.0 ** w_exp, dtype=torch.float64)
    if w_shift:
        rs = rs * torch.exp2(-(torch.arange(N) % 4).double())
    W64 = Wi * rs[:, None]
    nb = int(round(bias_max / bias_step))
    bias64 = _ints(g, (N,), -nb, nb) * bias_step
    A, W, bias = A64.to(torch.bfloat16), W64.to(torch.bfloat16), bias64.float()
    assert torch.equal(A.double(), A64) and torch.equal(W.double(), W64) and torch.equal(bias.double(), bias64)
    return SimpleNamespace(M=M, N=N, K=K, amp=amp, A=A, W=W, bias=bias, A64=A64, W64=W64, bias64=bias64, row_scale=rs)


def _e4m3_bytes(x64):
    b = x64.float().to(torch.float8_e4m3fn)
    assert torch.equal(b.double(), x64), "value without an e4m3 encoding"
    return b.view(torch.uint8).contiguous()


def exact_pair_fp8(M, N, K, seed, mx=False):
    """fp8 operands: A8 [M][K], W8 [N][K] uint8 e4m3 encodings of {0, +-1, +-2, +-3, +-4, +-6, +-8}, row scales
    a_scale [M], w_scale [N] powers of two in [2^-3, 2^2] varied by row, bias as exact_pair.  mx: also E8M0 block
    scales mx [M][K/32] (natural order) in [125, 129], x = q * 2^(s - 127); A64 is then the block-scaled matrix and
    a_scale is not part of the product.  sum |a||w| <= EXACT_SUM before any scale (asserted).  A64 / W64 are the
    dequantised float64 matrices: the reference is A64 @ W64.T (+ bias)."""
    assert K % 128 == 0 and 64 * K <= EXACT_SUM
    g = _gen(seed)
    vals = torch.tensor(sorted({s * v for v in FP8_VALUES for s in (1.0, -1.0)}), dtype=torch.float64)
    Aq = vals[torch.randint(0, len(vals), (M, K), generator=g)]
    Wq = vals[torch.randint(0, len(vals), (N, K), generator=g)]        # (sum |a||w| <= 64 K <= EXACT_SUM)
    a_scale64 = torch.exp2(((torch.arange(M) * 5 + int(torch.randint(0, 6, (1,), generator=g))) % 6 - 3).double())
    w_scale64 = torch.exp2(((torch.arange(N) * 7 + int(torch.randint(0, 6, (1,), generator=g))) % 6 - 3).double())
    bias64 = _ints(g, (N,), -128, 128) * 0.5
    out = SimpleNamespace(M=M, N=N, K=K, A8=_e4m3_bytes(Aq), W8=_e4m3_bytes(Wq), a_scale=a_scale64.float(),
                          w_scale=w_scale64.float(), bias=bias64.float(), bias64=bias64, Aq64=Aq, Wq64=Wq,
                          W64=Wq * w_scale64[:, None], mx=None)
    if mx:
        s = torch.randint(125, 130, (M, K // 32), generator=g, dtype=torch.int64)
        out.mx = s.to(torch.uint8)
        out.A64 = (Aq.view(M, K // 32, 32) * torch.exp2((s - 127).double())[..., None]).view(M, K)
    else:
        out.A64 = Aq * a_scale64[:, None]
    return out


def mx_frag_order(mx):
    """The fp8 GEMV's scale layout [M][4][K/128] (block 4c + g at [m][g][c]) of natural-order scales [M][K/32]."""
    M, nb = mx.shape
    return mx.view(M, nb // 4, 4).permute(0, 2, 1).contiguous().view(-1)


def _poison_value(dtype):
    return 0x7F if dtype == torch.uint8 else float("nan")       # 0x7F: the e4m3 NaN


def poisoned(A, W, M_pad=3, K_pad=8):
    """The same pair embedded in larger allocations: A with lda = K + K_pad and NaN in the pad columns and in M_pad rows
    after row M; W (row-major only -- a packed W has no pad) with NaN rows after row N.  Returns the views (A_view,
    W_view), on the inputs' device: every byte a kernel may touch is inside an allocation, so nothing can fault, and
    an over-read that reaches a result turns it NaN."""
    M, K = A.shape
    N = W.shape[0]
    bigA = torch.full((M + M_pad, K + K_pad), _poison_value(A.dtype), dtype=A.dtype, device=A.device)
    bigA[:M, :K] = A
    bigW = torch.full((N + M_pad, W.shape[1]), _poison_value(W.dtype), dtype=W.dtype, device=W.device)
    bigW[:N] = W
    return bigA[:M, :K], bigW[:N]


GELU_SIGMA = 2.8             # gelu_pair sizes row n so that rms(A) * |W[n]| lies in (GELU_SIGMA / 2, GELU_SIGMA]


def _gelu_row_exponents(A64, W64, room):
    """Per row n of W the exponent j[n] (W[n] * 2^-j[n]) that brings the spread rms(A) * |W[n]| of the row's
    pre-activations into (GELU_SIGMA / 2, GELU_SIGMA] -- the same for one row of A as for thousands -- raised, where a
    row's largest pre-activation still exceeds `room`, until it fits."""
    sigma = A64.pow(2).mean().sqrt() * W64.pow(2).sum(1).sqrt()
    j = torch.ceil(torch.log2(sigma.clamp_min(1e-300) / GELU_SIGMA))
    top = (A64 @ W64.t()).abs().amax(0) * torch.exp2(-j)
    return j + torch.ceil(torch.log2(top.clamp_min(room) / room))


def _gate_share(pre, mul):
    gate = pre.view(pre.shape[0], -1, 2, 16)[:, :, 0] if mul else pre
    return float(((gate >= -4.0) & (gate <= -0.5)).double().mean())


def gelu_pair(M, N, K, seed, mul=False, A64=None, room=None, **kw):
    """An exact_pair whose W rows each carry one more power of two (_gelu_row_exponents), so that every pre-activation
    A @ W.T (+ bias) satisfies |x| <= GELU_MAX and at least 10 % of the (gate) pre-activations lie in [-4, -0.5],
    where tanh- and erf-GELU differ by more than a bf16 step.  Both conditions are asserted.  mul: the gelu(gate) * up
    form -- W rows are the 16-gate / 16-up interleave, N counts both, there is no bias and the up pre-activations obey
    the same bound.  A64: the rows that will stand in for A (x built by a prologue); room: a tighter bound on
    |A @ W.T| for a caller that alters W afterwards."""
    p = exact_pair(M, N, K, seed, bias_step=0.25, bias_max=1.0, **kw)
    if mul:
        p.bias = p.bias64 = None
    if A64 is not None:
        p.A64, p.A = A64, None
    j = _gelu_row_exponents(p.A64, p.W64, room or GELU_MAX - (0.0 if mul else 1.0))
    p.W64 = p.W64 * torch.exp2(-j)[:, None]
    p.W = p.W64.to(torch.bfloat16)
    assert torch.equal(p.W.double(), p.W64)
    p.row_scale = p.row_scale * torch.exp2(-j)
    pre = ref_linear(p)
    p.share = _gate_share(pre, mul)
    assert float(pre.abs().max()) <= GELU_MAX and p.share >= 0.10, (float(pre.abs().max()), p.share)
    return p


def gelu_pair_fp8(M, N, K, seed):
    """An exact_pair_fp8 for the gelu(gate) * up epilogue (16-gate / 16-up interleaved rows, no bias): w_scale[n] is
    the power of two of _gelu_row_exponents (so it may fall below the 2^-3 of exact_pair_fp8); the conditions of
    gelu_pair are asserted."""
    p = exact_pair_fp8(M, N, K, seed)
    p.bias = p.bias64 = None
    j = _gelu_row_exponents(p.A64, p.Wq64, GELU_MAX)
    p.w_scale = torch.exp2(-j).float()
    p.W64 = p.Wq64 * torch.exp2(-j)[:, None]
    pre = ref_linear(p)
    p.share = _gate_share(pre, True)
    assert float(pre.abs().max()) <= GELU_MAX and p.share >= 0.10, (float(pre.abs().max()), p.share)
    return p


def rope_tables_exact(P, D, seed):
    """cos / sin fp32 tables [P][D/2] whose (cos, sin) entries come from ROPE_ENTRIES, chosen per (position, pair) from
    the seed: x*c - y*s and y*c + x*s are then exact in fp32 for exact accumulators (|x|, |y| <= EXACT_SUM with a
    2^-3 grid: 24 bits).  Not rotations -- the kernels take the tables as data."""
    ent = torch.tensor(ROPE_ENTRIES, dtype=torch.float32)
    idx = torch.randint(0, len(ROPE_ENTRIES), (P, D // 2), generator=_gen(seed))
    return ent[idx, 0].contiguous(), ent[idx, 1].contiguous()


def norm_rows_exact(M, K, nsplit, seed, use_fx=False, with_resid=True):
    """Inputs of the RMSNorm prologue (pro_mode 1) whose normalised rows are known exactly:
    v = resid + sum(partials) (+ fx / 2^32 with use_fx) has every entry +-c_m, c_m in NORM_C per row.  The partials
    [max(nsplit, 1)][M][K] (only the first nsplit are summed) are random integers and resid (or, with with_resid False,
    fx alone) is what is left, so dropping or repeating a slab breaks the pattern.  1 + norm_w is drawn from NORM_W1.
    The mean square is c_m^2, so with eps = 1e-6 v * rstd * (1 + w) lies within 2e-6 relative of +-(1 + w): x, the bf16
    rounding (half step 2e-3), is exactly +-(1 + w) whatever the last bits of the kernel's rsqrt.
    Returns resid (fp32 or None), partials fp32, fx (int64 or None), norm_w fp32, v64, x64."""
    g = _gen(seed)
    c = torch.tensor(NORM_C, dtype=torch.float64)[(torch.arange(M) + int(torch.randint(0, 4, (1,), generator=g))) % 4]
    sign = _ints(g, (M, K), 0, 1) * 2 - 1
    v64 = sign * c[:, None]
    part64 = _ints(g, (max(nsplit, 1), M, K), -16, 16)
    rest = v64 - part64[:nsplit].sum(0)
    fx = resid = None
    if use_fx:
        fxv = rest if not with_resid else _ints(g, (M, K), -32, 32) * 0.25
        fx = (fxv * 2.0 ** 32).to(torch.int64)
        assert torch.equal(fx.double(), fxv * 2.0 ** 32)
        rest = rest - fxv
    if with_resid or not use_fx:
        resid = rest.float()
        assert torch.equal(resid.double(), rest)
    w1 = torch.tensor(NORM_W1, dtype=torch.float64)[torch.randint(0, 4, (K,), generator=g)]
    return SimpleNamespace(M=M, K=K, nsplit=nsplit, resid=resid, partials=part64.float(), fx=fx,
                           norm_w=(w1 - 1.0).float(), v64=v64, x64=sign * w1[None, :], c=c)


def rmsnorm64(v64, norm_w, eps=1e-6):
    """The float64 RMSNorm v * rsqrt(mean(v^2) + eps) * (1 + w)."""
    return v64 * torch.rsqrt(v64.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + norm_w.double())


# ---------------------------------------------------------------------------------------------- references (float64)
def ref_linear(p, bias=True):
    out = p.A64 @ p.W64.t()
    if bias and getattr(p, "bias64", None) is not None:
        out = out + p.bias64.to(out.device)
    return out


def gelu64(x):
    """tanh-GELU as x / (1 + exp(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3).  (0.5 x (1 + tanh u) cancels in the negative
    tail: in float64 it is itself wrong by tens of percent at x = -8.)"""
    x = x.double()
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x / (1.0 + torch.exp(-2.0 * u))


def gelu_erf64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_mul64(pre, gelu=gelu64):
    """gelu(gate) * up of pre-activations [M][N] whose columns are the 16-gate / 16-up interleave -> [M][N/2]."""
    M, N = pre.shape
    g = pre.reshape(M, N // 32, 2, 16)
    return (gelu(g[:, :, 0]) * g[:, :, 1].double()).reshape(M, N // 2)


def dec_koff(k, d, D):
    """Element offset of (key k, dim d) inside one (batch, kv head) of the decode-order K copy (include/pghip.h kd;
    csrc/attn_common.h): [32-key block][half h][D/8 chunk][row r][8], key 32 blk + 8 q + 4 h + j <-> row 4 q + j."""
    blk, kk = k >> 5, k & 31
    h, r = (kk >> 2) & 1, ((kk >> 3) << 2) | (kk & 3)
    return (((blk * 2 + h) * (D >> 3) + (d >> 3)) * 16 + r) * 8 + (d & 7)


def dec_voff(k, d, D):
    """... of the decode-order V copy: [32-key block][D/16 tile][key group of 8][dim in tile][key in group]."""
    blk, kk = k >> 5, k & 31
    return (((blk * (D >> 4) + (d >> 4)) * 4 + (kk >> 3)) * 16 + (d & 15)) * 8 + (kk & 7)


def decode_copies(kc, vtc, Hkv):
    """numpy (kd, vd) [B][Hkv][Smax][D] of a canonical cache kc [B][Smax][Hkv*D], vtc [B][Hkv*D][Smax], element by
    element from dec_koff / dec_voff."""
    B, S, KV = kc.shape
    D = KV // Hkv
    k, d = np.meshgrid(np.arange(S), np.arange(D), indexing="ij")
    ko, vo = dec_koff(k, d, D).ravel(), dec_voff(k, d, D).ravel()
    kd = np.zeros((B, Hkv, S * D), dtype=kc.dtype)
    vd = np.zeros((B, Hkv, S * D), dtype=kc.dtype)
    for h in range(Hkv):
        kd[:, h, ko] = kc[:, :, h * D:(h + 1) * D].reshape(B, S * D)
        vd[:, h, vo] = vtc[:, h * D:(h + 1) * D, :].transpose(0, 2, 1).reshape(B, S * D)
    return kd.reshape(B, Hkv, S, D), vd.reshape(B, Hkv, S, D)


def rope_row_perm(D):
    """Row order inside one D-wide head block of the fused q|k|v weight: 16-row tile t holds dims 8t..8t+7 then
    D/2 + 8t..D/2 + 8t + 7 (pghip/weights.py rope_row_perm; restated so the reference does not lean on it)."""
    idx = []
    for t in range(D // 16):
        idx += [8 * t + j for j in range(8)] + [D // 2 + 8 * t + j for j in range(8)]
    return np.array(idx)


def bf16_rne(x64):
    """float64 -> the nearest bfloat16 value (ties to even), as float64: one rounding, by integer arithmetic on the
    bits (normal range only; zero stays zero)."""
    x64 = x64.double().contiguous()
    b = x64.view(torch.int64)
    b = b + ((1 << 44) - 1) + ((b >> 45) & 1)
    return (b & ~((1 << 45) - 1)).view(torch.float64)


def bf16_trunc(x64):
    x64 = x64.double().contiguous()
    return (x64.view(torch.int64) & ~((1 << 45) - 1)).view(torch.float64)


def qkv_rope_ref(acc64, pos, cos_t, sin_t, *, L, Hq, Hkv, D, smax, slots, fill, round_input=False):
    """The fused q|k|v epilogue on exact accumulators acc64 [M][(Hq + 2 Hkv) D] in ORIGINAL (unpermuted) column order:
    rotate pair (d, d + D/2) of every q and k head with the tables' row pos[m], round once to bf16, place k at
    kc[b][slot][kvh*D + d], v at vtc[b][kvh*D + d][slot], b = m // L, slot = slots[m] (a slot outside [0, smax) is
    not appended), and the decode-order copies through dec_koff / dec_voff.  Everything not written holds `fill`.
    round_input: the accumulators are first rounded to bf16 (pg_rope_kv_write reads a bf16 q|k|v).
    Returns float64 numpy arrays q [M][Hq*D], kc [B][smax][Hkv*D], vtc [B][Hkv*D][smax], kd, vd [B][Hkv][smax][D]."""
    acc = acc64.double().cpu()
    if round_input:
        acc = bf16_rne(acc)
    M = acc.shape[0]
    B, half = M // L, D // 2
    x = acc.view(M, Hq + 2 * Hkv, D)
    c = cos_t.double()[pos.long()][:, None, :]
    s = sin_t.double()[pos.long()][:, None, :]
    r = x[:, :Hq + Hkv]
    x1, x2 = r[..., :half], r[..., half:]
    rot = bf16_rne(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)).numpy()
    v = bf16_rne(x[:, Hq + Hkv:]).numpy()
    q = rot[:, :Hq].reshape(M, Hq * D)
    kc = np.full((B, smax, Hkv * D), float(fill))
    vtc = np.full((B, Hkv * D, smax), float(fill))
    kd = np.full((B, Hkv, smax * D), float(fill))
    vd = np.full((B, Hkv, smax * D), float(fill))
    dd = np.arange(D)
    for m in range(M):
        b, slot = m // L, int(slots[m])
        if not 0 <= slot < smax:
            continue
        kc[b, slot] = rot[m, Hq:].reshape(-1)
        vtc[b, :, slot] = v[m].reshape(-1)
        for h in range(Hkv):
            kd[b, h, dec_koff(slot, dd, D)] = rot[m, Hq + h]
            vd[b, h, dec_voff(slot, dd, D)] = v[m, h]
    return q, kc, vtc, kd.reshape(B, Hkv, smax, D), vd.reshape(B, Hkv, smax, D)


# ---------------------------------------------------------------------------------------------- checkers
def _f32_exact(ref64):
    r = ref64.double()
    f = r.float()
    if not torch.equal(f.double(), r):
        raise AssertionError("the float64 reference is not fp32-representable: the exactness premise fails")
    return f


def exact_f32(got, ref64):
    """Per-element mask: got (fp32) has exactly the bits of ref64 (which must be fp32-representable)."""
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (got.dtype, got.shape, ref64.shape)
    return got.contiguous().view(torch.int32) == _f32_exact(ref64).contiguous().view(torch.int32)


def exact_bf16(got, ref64):
    """Per-element mask: got (bf16) has exactly the bits of the RNE rounding of ref64 (fp32-representable)."""
    assert got.dtype == torch.bfloat16 and got.shape == ref64.shape, (got.dtype, got.shape, ref64.shape)
    want = _f32_exact(ref64).to(torch.bfloat16)
    assert torch.equal(want.double(), bf16_rne(ref64))
    return got.contiguous().view(torch.int16) == want.contiguous().view(torch.int16)


def within_bf16(got, ref64, delta):
    """Per-element mask: bf16(ref (1 - delta)) <= got <= bf16(ref (1 + delta)), ordered by value -- got is the RNE
    rounding of some y within delta of the reference.  No element is excluded and there is no absolute floor: a zero
    reference demands a zero.  Every non-zero reference must be a normal fp32 number (asserted)."""
    assert got.dtype == torch.bfloat16 and got.shape == ref64.shape, (got.dtype, got.shape, ref64.shape)
    r = ref64.double()
    assert bool(((r == 0) | (r.abs() >= 2.0 ** -126)).all()) and bool(r.abs().max() < 2.0 ** 127)
    a, b = bf16_rne(r * (1.0 - delta)), bf16_rne(r * (1.0 + delta))
    g = got.double()
    return (g >= torch.minimum(a, b)) & (g <= torch.maximum(a, b))


def assert_all(ok, what=""):
    """Every element of the mask holds; the message names the count and the first failing indices."""
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements fail, first at {bad[:8].tolist()}")
