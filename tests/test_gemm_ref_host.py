"""CPU-only checks of tests/gemm_ref.py: the builders keep the conditions that make a GEMM exact, the exact outputs
exercise bf16 rounding (census), the checkers accept an fp32 emulation of the kernel's own GELU formula and reject
each deliberately wrong epilogue that the max-error metric of test_kernels_gpu.py lets through."""
import math

import numpy as np
import pytest
import torch

import gemm_ref as R

KS = (64, 192, 2048, 16384)
KS_FP8 = (128, 384, 2048, 16384)          # the fp8 GEMMs take K % 128 == 0


def _is_bf16(x64):
    return torch.equal(x64.to(torch.bfloat16).double(), x64)


@pytest.mark.parametrize("K", KS)
def test_exact_pair_conditions(K):
    """Operands bf16-exact integers (times the row's power of two), sum |a||w| <= 2^20, bias multiples of 0.5 within
    64, every output and every output + bias fp32-exact."""
    p = R.exact_pair(5, 48, K, seed=K)
    assert p.amp == 8 and R.default_amp(K) == 8 and R.default_amp(4 * 16384) == 4
    assert _is_bf16(p.A64) and _is_bf16(p.W64) and p.A.dtype == torch.bfloat16
    assert float(p.A64.abs().max()) <= p.amp and torch.equal(p.A64, p.A64.round())
    Wi = p.W64 / p.row_scale[:, None]
    assert torch.equal(Wi, Wi.round()) and float(Wi.abs().max()) <= p.amp
    assert torch.equal(p.row_scale, torch.exp2(-(torch.arange(48) % 4).double()))
    assert float((p.A64.abs() @ Wi.abs().t()).max()) <= R.EXACT_SUM
    assert float(p.bias64.abs().max()) <= 64 and torch.equal(p.bias64 * 2, (p.bias64 * 2).round())
    for ref in (R.ref_linear(p), R.ref_linear(p, bias=False)):
        assert torch.equal(ref.float().double(), ref)
    q = R.exact_pair(5, 48, K, seed=K)
    assert torch.equal(p.A, q.A) and torch.equal(p.W, q.W) and torch.equal(p.bias, q.bias)      # seeded
    assert not torch.equal(p.A, R.exact_pair(5, 48, K, seed=K + 1).A)
    with pytest.raises(AssertionError):
        R.exact_pair(2, 16, 4 * 16384, seed=0, amp=8)


@pytest.mark.parametrize("K", KS_FP8)
@pytest.mark.parametrize("mx", [False, True])
def test_exact_pair_fp8_conditions(K, mx):
    """Bytes are e4m3 encodings of the allowed set, scales powers of two in [2^-3, 2^2] varied by row, E8M0 block
    scales in [125, 129], sum |a||w| <= 2^20 before the scales, the scaled outputs fp32-exact."""
    p = R.exact_pair_fp8(9, 48, K, seed=K, mx=mx)
    allowed = {s * v for v in R.FP8_VALUES for s in (1.0, -1.0)}
    for b, q in ((p.A8, p.Aq64), (p.W8, p.Wq64)):
        assert b.dtype == torch.uint8 and torch.equal(b.view(torch.float8_e4m3fn).double(), q)
        assert set(q.unique().tolist()) <= allowed
    assert float((p.Aq64.abs() @ p.Wq64.abs().t()).max()) <= R.EXACT_SUM
    for s in (p.a_scale, p.w_scale):
        e = torch.log2(s.double())
        assert torch.equal(e, e.round()) and float(e.min()) >= -3 and float(e.max()) <= 2 and s.unique().numel() > 1
    if mx:
        assert p.mx.dtype == torch.uint8 and p.mx.shape == (9, K // 32)
        assert int(p.mx.min()) >= 125 and int(p.mx.max()) <= 129 and p.mx.unique().numel() > 1
        assert torch.equal(p.A64, (p.Aq64.view(9, K // 32, 32) *
                                   torch.exp2(p.mx.double() - 127)[..., None]).view(9, K))
        fr = R.mx_frag_order(p.mx).view(9, 4, K // 128)
        assert all(int(fr[2, g, c]) == int(p.mx[2, 4 * c + g]) for g in range(4) for c in range(K // 128))
    else:
        assert torch.equal(p.A64, p.Aq64 * p.a_scale.double()[:, None])
    ref = R.ref_linear(p)
    assert torch.equal(ref.float().double(), ref)


def test_poisoned_views():
    p = R.exact_pair(5, 48, 64, seed=1)
    A, W = R.poisoned(p.A, p.W, M_pad=2, K_pad=8)
    assert torch.equal(A, p.A) and torch.equal(W, p.W) and A.stride(0) == 72 and W.stride(0) == 64
    bigA = torch.as_strided(A, (7, 72), (72, 1))
    assert bool(bigA[:5, 64:].isnan().all()) and bool(bigA[5:].isnan().all())
    assert bool(torch.as_strided(W, (50, 64), (64, 1))[48:].isnan().all())
    f = R.exact_pair_fp8(5, 48, 128, seed=1)
    A8, _ = R.poisoned(f.A8, f.W8)
    assert bool(torch.as_strided(A8, (8, 136), (136, 1))[5:].view(torch.float8_e4m3fn).float().isnan().all())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mul", [False, True])
def test_gelu_pair_conditions(K, mul):
    p = R.gelu_pair(24, 96, K, seed=K + 7, mul=mul)
    pre = R.ref_linear(p)
    assert float(pre.abs().max()) <= R.GELU_MAX and p.share >= 0.10
    assert _is_bf16(p.W64) and (p.bias is None) == mul
    assert torch.equal(pre.float().double(), pre)


@pytest.mark.parametrize("M", [1, 16])
def test_gelu_pair_behind_a_prologue_and_for_packed_weights(M):
    """The options the packed decode cases use: rows standing in for A (a norm prologue's +-(1 + w)), a tighter bound
    that leaves room for planted zeros, and weights without a zero; one row of A spreads as well as many."""
    n = R.norm_rows_exact(M, 1024, 0, seed=3)
    p = R.gelu_pair(M, 96, 1024, seed=4, mul=True, A64=n.x64, room=R.GELU_MAX - 1, w_nonzero=True)
    pre = R.ref_linear(p)
    assert p.A64 is n.x64 and float(pre.abs().max()) <= R.GELU_MAX - 1 and p.share >= 0.10
    assert bool((p.W64 != 0).all()) and _is_bf16(p.W64)


@pytest.mark.parametrize("M,K", [(9, 256), (300, 128), (32, 2048)])
def test_gelu_pair_fp8_conditions(M, K):
    p = R.gelu_pair_fp8(M, 512, K, seed=M + K)
    pre = R.ref_linear(p)
    e = torch.log2(p.w_scale.double())
    assert torch.equal(e, e.round()) and p.bias is None
    assert torch.equal(p.W64, p.Wq64 * p.w_scale.double()[:, None]) and torch.equal(p.A8.view(torch.float8_e4m3fn)
                                                                                 .double(), p.Aq64)
    assert float(pre.abs().max()) <= R.GELU_MAX and p.share >= 0.10
    assert torch.equal(pre.float().double(), pre)


@pytest.mark.parametrize("D", [16, 32, 256])
def test_rope_tables_exact_entries(D):
    c, s = R.rope_tables_exact(40, D, seed=D)
    assert c.shape == s.shape == (40, D // 2) and c.dtype == torch.float32
    seen = set(zip(c.flatten().tolist(), s.flatten().tolist()))
    assert seen <= set(R.ROPE_ENTRIES) and len(seen) == len(R.ROPE_ENTRIES)


@pytest.mark.parametrize("K", (2048, 16384))
def test_census_of_exact_outputs(K):
    """If these fail, the BF16 cases would not see a rounding-mode error: enough outputs must need rounding, sit on
    exact ties, and round differently under truncation."""
    p = R.exact_pair(24, 96, K, seed=K + 3)
    ref = R.ref_linear(p)
    rne, tr = R.bf16_rne(ref), R.bf16_trunc(ref)
    assert torch.equal(rne, ref.float().to(torch.bfloat16).double())          # the bit-trick rounding is torch's
    inexact = float((rne != ref).double().mean())
    up = torch.nextafter(tr.to(torch.bfloat16), (tr.sign() * math.inf).to(torch.bfloat16)).double()
    ties = float(((ref != tr) & ((ref - tr).abs() == (up - ref).abs())).double().mean())
    trunc_differs = float((tr != rne).double().mean())
    print(f"K {K}: not bf16 {inexact:.3f}, ties {ties:.3f}, truncation differs {trunc_differs:.3f}")
    assert inexact >= 0.25 and ties >= 0.05 and trunc_differs >= 0.20


def _kernel_gelu_f32(x, c3=0.044715):
    """gelu_tanh of csrc/common.h in torch fp32: x * (1 / (1 + exp2(-2.88539 u)))."""
    x = x.float()
    u = 0.7978845608028654 * (x + c3 * x * x * x)
    return x * (1.0 / (1.0 + torch.exp2(-2.8853900817779268 * u)))


@pytest.mark.parametrize("mul", [False, True])
def test_gelu_checker_accepts_the_kernel_formula_and_rejects_each_mutation(mul):
    p = R.gelu_pair(150, 320, 192, seed=11, mul=mul)
    pre = R.ref_linear(p)
    ref = R.gelu_mul64(pre) if mul else R.gelu64(pre)

    def emu(g):
        if not mul:
            return g(pre.float())
        x = pre.float().view(150, 10, 2, 16)
        return (g(x[:, :, 0]) * x[:, :, 1]).reshape(150, 160)
    good = emu(_kernel_gelu_f32)
    R.assert_all(R.within_bf16(good.to(torch.bfloat16), ref, R.GELU_DELTA), "fp32 emulation of gelu_tanh")
    shares = {}
    for name, got in (("erf", emu(lambda x: R.gelu_erf64(x).float()).to(torch.bfloat16)),
                      ("cubic 0.04", emu(lambda x: _kernel_gelu_f32(x, 0.04)).to(torch.bfloat16)),
                      ("truncation", R.bf16_trunc(good.double()).to(torch.bfloat16))):
        shares[name] = float((~R.within_bf16(got, ref, R.GELU_DELTA)).double().mean())
    print("rejected shares:", shares)
    assert all(s >= 0.05 for s in shares.values()), shares
    # the tanh form the references avoid: wrong by tens of percent in the negative tail, in float64
    x = torch.tensor([-8.0], dtype=torch.float64)
    u = math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)
    assert abs(float(0.5 * x * (1 + torch.tanh(u)) / R.gelu64(x)) - 1) > 0.1


def test_exact_checkers_reject_a_scaled_row_and_a_dropped_k():
    p = R.exact_pair(100, 300, 2048, seed=5)
    ref = R.ref_linear(p)
    good = ref.float()
    assert bool(R.exact_f32(good, ref).all()) and bool(R.exact_bf16(good.to(torch.bfloat16), ref).all())
    bad = good.clone()
    bad[-1] *= 1.01
    ok = R.exact_bf16(bad.to(torch.bfloat16), ref)
    print("last row x 1.01: rejected share of that row", float((~ok[-1]).double().mean()))
    assert bool(ok[:-1].all()) and float((~ok[-1]).double().mean()) >= 0.5
    short = (p.A64[:, :-1] @ p.W64[:, :-1].t() + p.bias64).float()
    assert float((~R.exact_f32(short, ref)).double().mean()) >= 0.5
    trunc = R.bf16_trunc(ref).to(torch.bfloat16)
    assert float((~R.exact_bf16(trunc, ref)).double().mean()) >= 0.2
    with pytest.raises(AssertionError):                     # a reference outside fp32 is a broken premise, not a pass
        R.exact_f32(good, ref + 2.0 ** -40)
    with pytest.raises(AssertionError):
        R.assert_all(ok, "scaled row")
    z = torch.zeros(3, dtype=torch.float64)                 # a zero reference demands a zero, of either sign
    assert bool(R.within_bf16(torch.tensor([0.0, -0.0, 1e-30], dtype=torch.bfloat16), z, R.GELU_DELTA)[:2].all())
    assert not bool(R.within_bf16(torch.tensor([0.0, -0.0, 1e-30], dtype=torch.bfloat16), z, R.GELU_DELTA)[2])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nsplit,use_fx,with_resid", [(0, False, True), (1, False, True), (4, False, True),
                                                      (4, True, True), (0, True, False)])
def test_norm_rows_exact(K, nsplit, use_fx, with_resid):
    """The float64 RMSNorm at eps = 1e-6 rounds to exactly +-(1 + w); dropping (or repeating) a slab changes x."""
    n = R.norm_rows_exact(5, K, nsplit, seed=K + nsplit, use_fx=use_fx, with_resid=with_resid)

    def total(slabs):
        v = n.partials[:slabs].double().sum(0)
        if n.resid is not None:
            v = v + n.resid.double()
        if n.fx is not None:
            v = v + n.fx.double() / 2.0 ** 32
        return v
    v = total(nsplit)
    assert torch.equal(v, n.v64) and torch.equal(v.abs(), n.c[:, None].expand(5, K))
    assert set((1 + n.norm_w.double()).unique().tolist()) <= set(R.NORM_W1)
    x = R.rmsnorm64(v, n.norm_w)
    assert float(((x - n.x64).abs() / n.x64.abs()).max()) < 4e-6
    assert torch.equal(R.bf16_rne(x), n.x64)
    assert (n.resid is None) == (not with_resid) and (n.fx is None) == (not use_fx)
    if nsplit:
        for slabs in (nsplit - 1, nsplit + 1 if nsplit < n.partials.shape[0] else nsplit - 1):
            assert not torch.equal(R.bf16_rne(R.rmsnorm64(total(slabs), n.norm_w)), n.x64)


def test_cache_placement_reference_agrees_with_decode_cache_pack():
    """decode_copies (element by element from dec_koff / dec_voff) against ops.decode_cache_pack's reshapes, and
    qkv_rope_ref's own placement of one appended row, on the CPU."""
    from pghip import ops
    from pghip.weights import rope_row_perm
    B, S, Hkv, D = 2, 64, 2, 32
    g = torch.Generator().manual_seed(3)
    kc = torch.randint(-100, 100, (B, S, Hkv * D), generator=g).to(torch.bfloat16)
    vtc = torch.randint(-100, 100, (B, Hkv * D, S), generator=g).to(torch.bfloat16)
    kd_t, vd_t = ops.decode_cache_pack(kc, vtc, Hkv)
    kd, vd = R.decode_copies(kc.float().numpy(), vtc.float().numpy(), Hkv)
    assert np.array_equal(kd, kd_t.float().numpy()) and np.array_equal(vd, vd_t.float().numpy())
    Hq, L, M = 2, 3, 6
    acc = torch.randint(-50, 50, (M, (Hq + 2 * Hkv) * D), generator=g).double()
    pos = torch.arange(M, dtype=torch.int32) % 5
    cos_t, sin_t = R.rope_tables_exact(8, D, seed=2)
    slots = [40 + m % L for m in range(M)]
    slots[5] = S                                             # past the cache: not appended
    q, k2, vt2, kd2, vd2 = R.qkv_rope_ref(acc, pos, cos_t, sin_t, L=L, Hq=Hq, Hkv=Hkv, D=D, smax=S, slots=slots,
                                          fill=0.0)
    kd_t, vd_t = ops.decode_cache_pack(torch.from_numpy(k2), torch.from_numpy(vt2), Hkv)
    assert np.array_equal(kd2, kd_t.numpy()) and np.array_equal(vd2, vd_t.numpy())
    assert np.count_nonzero(k2[1, 42]) == 0 and np.count_nonzero(k2[1, 41]) > 0 and np.count_nonzero(k2[:, :40]) == 0
    # one element by hand: q head 1, pair (d = 3, d + D/2), row 4
    x1, x2 = float(acc[4, D + 3]), float(acc[4, D + 3 + D // 2])
    c, s = float(cos_t[pos[4], 3]), float(sin_t[pos[4], 3])
    assert q[4, D + 3] == float(R.bf16_rne(torch.tensor([x1 * c - x2 * s]))[0])
    assert q[4, D + 3 + D // 2] == float(R.bf16_rne(torch.tensor([x2 * c + x1 * s]))[0])
    assert vt2[1, D + 5, 40 + 1] == float(acc[4, (Hq + Hkv + 1) * D + 5])
    assert list(R.rope_row_perm(32)) == rope_row_perm(32).tolist()
