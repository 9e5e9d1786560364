"""Ragged batches: prompts of different lengths in one generate call (per-row kv lengths from the kernels up).

The contract: each row of a right-padded batch generates what that row generates alone, unpadded, at B = 1.
Bounds (the project's existing ones): scaled max error on logits < 3e-2 (test_engine_gpu.TOL), on kernel outputs against
fp32 torch < 2e-2 (test_kernels_gpu), greedy ids equal where the oracle's top-1 margin exceeds 0.1.  The inputs and the
oracle references live in tests/ragged_ref.py (computed once per request, shared by the tests).

Length sets follow the rules there: a row of one or two text tokens (18 / 19 keys), a multiple of 64 and that plus one,
a row that crosses a multiple of 32 within the decoded steps, and a longest row at least two 64-key blocks longer than
the shortest, so whole key blocks -- and with key splits whole splits -- are empty for the short rows."""
import numpy as np
import pytest
import torch

import ragged_ref as R

pytestmark = pytest.mark.gpu

TOL = 3e-2          # logits (test_engine_gpu.TOL)
KTOL = 2e-2         # kernel outputs against fp32 torch (test_kernels_gpu)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).cuda()


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def ragged_lens(B: int, L: int):
    """B lengths <= L by the module's rules: 19, L itself, a multiple of 64 and that plus 1, then fillers."""
    base = [19, L, 64, 65, 18, (L // 64) * 64, (L // 64) * 64 + 1 if (L // 64) * 64 + 1 <= L else L - 1, 31, 33, 128]
    out = [min(x, L) for x in base]
    while len(out) < B:
        out.append(1 + (37 * len(out)) % L)
    assert L - 19 >= 128, "the longest row must be two 64-key blocks longer than the shortest"
    return out[:B]


def sharpen(kc, lens):
    """Make an off-by-one in a row's length visible inside the 2e-2 bound: row b's last valid key and all its stale
    keys get 3x the norm, so dropping the one or admitting the first of the others moves the softmax grossly (one key
    of weight 1 / len_b among equals would hide below the bound from 64 keys on)."""
    for b, n in enumerate(lens):
        kc[b, n - 1:] *= 3
    return kc


def _attn_ref_row(q, k, v, scale):
    """fp32 softmax attention of one batch row: q [nh][Lq][hd], k / v [nh][Lk][hd]."""
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    return torch.softmax(s, -1) @ v.float()


# ------------------------------------------------------------------------------------------------ 1. prefill kernel
def _prefill_case(B, L, nh, nkv, hd, nks=0, fallback=False, seed=100):
    from pghip import ops
    lens = ragged_lens(B, L)
    Smax = max(320, (L + 8 + 63) // 64 * 64)
    kvd, g = nkv * hd, nh // nkv
    q = rnd(B * L, nh * hd, seed=seed)
    kc = sharpen(rnd(B, Smax, kvd, seed=seed + 1), lens)    # every row finite: stale values past each row's length
    vtc = rnd(B, kvd, Smax, seed=seed + 2)
    args = (q, nh * hd, None, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax)
    kw = dict(B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5)
    if nks:
        no, nml = ops.prefill_split_workspace(B, L, nh, nkv, hd, nks)
        kw.update(nsplit=nks, part_o=torch.full((no,), float("nan"), device="cuda"),
                  part_ml=torch.full((nml,), float("nan"), device="cuda"))
    if fallback:    # an all-zero additive mask: the non-flash kernels (attn_kernel, or the LDS kernel from 1024 groups)
        mask = torch.zeros(B, L, L, device="cuda")
        kw.update(mask=mask, mask_bs=L * L, mask_rs=L)
    o = torch.full((B * L, nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.attention_rows(*args[:2], o, *args[3:], lkv_rows=i32(lens), **kw)
    assert torch.isfinite(o.float()).all(), "padding rows may compute anything finite"
    ov = o.view(B, L, nh, hd)
    qv = q.view(B, L, nh, hd)
    worst = 0.0
    for b, n in enumerate(lens):                            # one batch row at a time; only query rows < len_b
        kh = kc[b, :n].view(n, nkv, hd).transpose(0, 1).repeat_interleave(g, 0)
        vh = vtc[b, :, :n].view(nkv, hd, n).transpose(1, 2).repeat_interleave(g, 0)
        ref = _attn_ref_row(qv[b, :n].transpose(0, 1), kh, vh, hd ** -0.5)
        worst = max(worst, err(ov[b, :n].transpose(0, 1), ref))
    print(f"prefill rows B={B} L={L} hd={hd} nks={nks} fallback={fallback}: worst scaled error {worst:.4f}")
    assert worst < KTOL, (lens, worst)
    # every length equal to L: the same bits as the shared-length entry point
    full = torch.empty_like(o)
    same = torch.empty_like(o)
    ops.attention(*args[:2], full, *args[3:], **kw)
    ops.attention_rows(*args[:2], same, *args[3:], lkv_rows=i32([L] * B), **kw)
    assert torch.equal(full, same)


@pytest.mark.parametrize("B,L,nh,nkv,hd", [(4, 150, 4, 1, 32), (4, 150, 8, 2, 72), (4, 150, 8, 2, 128),
                                           (4, 150, 8, 1, 256), (5, 200, 8, 4, 256),
                                           (8, 600, 8, 8, 32)])               # 8-wave workgroups
def test_prefill_attention_rows_small_shapes(B, L, nh, nkv, hd):
    """pg_attention_rows, prefill: head_dim 32 / 72 / 128 / 256, MQA and GQA, against fp32 torch attention over each
    row's own first len_b keys, the cache rows past len_b holding finite stale values."""
    _prefill_case(B, L, nh, nkv, hd)


@pytest.mark.parametrize("B,L,nh,nkv,hd,nks", [(14, 300, 8, 1, 256, 0),       # 12-wave flash kernel
                                               (16, 1032, 8, 1, 256, 0),      # pt-448
                                               (32, 1000, 8, 1, 256, 0),      # 8 waves x 32 rows, 32-key blocks
                                               (4, 264, 8, 1, 256, 5),        # key splits: whole splits empty
                                               (2, 200, 4, 2, 64, 8), (1, 264, 8, 1, 256, 5)])
def test_prefill_attention_rows_flash_forms(B, L, nh, nkv, hd, nks):
    """The flash forms test_attention_cache_layout_prefill_and_decode reaches (12 waves, the pt-448 batch, 8 waves x 32
    rows on 32-key blocks) and the key-split form with pg_attention's own merge, on ragged lengths: a 19-key row leaves
    whole 64-key blocks -- and with 5 or 8 splits whole splits -- empty, and the merge must stay finite."""
    _prefill_case(B, L, nh, nkv, hd, nks=nks)


@pytest.mark.parametrize("B,L,nh,nkv,hd", [(4, 150, 8, 1, 256), (3, 150, 4, 2, 72), (8, 300, 8, 1, 32)])
def test_prefill_attention_rows_fallback_kernels(B, L, nh, nkv, hd):
    """The non-flash kernels take the per-row length too (an additive mask keeps pg_attention off the flash kernel: the
    one-wave kernel, and from 1024 sixteen-row groups the LDS-staged one, which zeroes V^T past len_b at staging)."""
    _prefill_case(B, L, nh, nkv, hd, fallback=True)


# ------------------------------------------------------------------------------------------------- 2. decode kernels
def _decode_lens(B: int, kcap: int):
    """Ragged kv lengths (keys each row attends): one shorter than 32, one within one key of kcap, blocks' edges."""
    base = [19, kcap - 1, 64, 65, kcap, 31, 33, 128, 129, 96]
    out = [min(x, kcap) for x in base]
    while len(out) < B:
        out.append(1 + (53 * len(out)) % kcap)
    return out[:B]


def _decode_ref(q, kc, vtc, lens, nh, nkv, hd):
    B, g = q.shape[0], nh // nkv
    rows = []
    for b, n in enumerate(lens):
        kh = kc[b, :n].view(n, nkv, hd).transpose(0, 1).repeat_interleave(g, 0)
        vh = vtc[b, :, :n].view(nkv, hd, n).transpose(1, 2).repeat_interleave(g, 0)
        rows.append(_attn_ref_row(q[b].view(nh, 1, hd), kh, vh, hd ** -0.5).reshape(nh * hd))
    return torch.stack(rows)


@pytest.mark.parametrize("B,nh,nkv,hd,kcap", [(2, 8, 1, 256, 256), (3, 8, 2, 256, 512), (8, 4, 1, 32, 128),
                                              (17, 8, 1, 256, 512), (3, 4, 1, 72, 128)])
def test_decode_split_attention_rows_and_combine(B, nh, nkv, hd, kcap):
    """pg_attention_rows in split mode + pg_attn_combine: row b attends Lkv + lkv_rows[b] keys.  Every split size the
    shared-length test walks (one-wave splits, the 2- / 4-wave LDS-merged ones at head_dim 256), with and without the
    decode-order copies (kcap), a stale-valued cache; equal lengths give the shared-length call's bits."""
    from pghip import ops
    kvd = nkv * hd
    lens = _decode_lens(B, kcap)
    q = rnd(B, nh * hd, seed=41)
    kc, vtc = sharpen(rnd(B, kcap, kvd, seed=42), lens), rnd(B, kvd, kcap, seed=43)
    ref = _decode_ref(q, kc, vtc, lens, nh, nkv, hd)
    dt = (hd + 15) // 16 * 16
    packed = hd % 32 == 0
    kd, vd = ops.decode_cache_pack(kc, vtc, nkv) if packed else (None, None)
    args = (q, nh * hd, None, nh * hd, kc, kcap * kvd, hd, kvd, vtc, kvd * kcap, hd * kcap, kcap)
    rows = i32([n - 1 for n in lens])                       # Lkv = 1 + the length before this token, as the engine
    same_n = kcap - 40
    for sk in (32, 64, 128, 256):
        ns = ((kcap + sk - 1) // sk + 3) // 4 * 4
        po = torch.empty(B * nkv * ns * 16 * dt, device="cuda")
        pml = torch.empty(B * nkv * ns * 16 * 2, device="cuda")
        for cap in (0, kcap):
            kw = dict(B=B, Lq=1, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, split_keys=sk, nsplit=ns, part_o=po,
                      part_ml=pml, kcap=cap, kd=kd if cap else None, vd=vd if cap else None)
            o = torch.full((B, nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
            ops.attention_rows(*args, Lkv=1, lkv_rows=rows, **kw)
            ops.attn_combine(po, pml, o, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=ns)
            assert err(o, ref) < KTOL, (sk, cap, lens)
            # equal lengths: bit-identical to the shared word
            a, b2 = torch.empty_like(o), torch.empty_like(o)
            ops.attention(*args, Lkv=1, lkv_dev=i32([same_n - 1]), **kw)
            ops.attn_combine(po, pml, a, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=ns)
            ops.attention_rows(*args, Lkv=1, lkv_rows=i32([same_n - 1] * B), **kw)
            ops.attn_combine(po, pml, b2, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=ns)
            assert torch.equal(a, b2), (sk, cap)


@pytest.mark.parametrize("B,nh,nkv,hd,kcap", [(2, 8, 1, 256, 256), (3, 8, 2, 256, 448), (8, 4, 1, 32, 128),
                                              (17, 8, 1, 256, 1216), (8, 8, 1, 256, 128)])
def test_attn_decode_rows_fused(B, nh, nkv, hd, kcap):
    """pg_attn_decode_rows over every plan test_attn_decode_fused walks (2 / 4 waves, 1..16 splits, several rounds; the
    staggered form where the plan has one; the fp8 row copy where the plan allows it): ragged lengths -- the ticketed
    merge meets splits that are empty for one row and full for the next -- against fp32 softmax attention, repeated
    calls bit-identical, tickets left zero, and equal lengths bit-identical to pg_attn_decode."""
    from pghip import ops
    kvd = nkv * hd
    lens = _decode_lens(B, kcap)
    q = rnd(B, nh * hd, seed=51)
    kc, vtc = sharpen(rnd(B, kcap, kvd, seed=52), lens), rnd(B, kvd, kcap, seed=53)    # stale rows past each length
    ref = _decode_ref(q, kc, vtc, lens, nh, nkv, hd)
    kd, vd = ops.decode_cache_pack(kc, vtc, nkv)
    cnt = torch.zeros(B * nkv, dtype=torch.int32, device="cuda")
    rows = i32(lens)
    nblk = kcap // 32
    plans = {ops.decode_plan(B, nkv, kcap)}
    for nw in (2, 4):
        for ns in (1, 3, 16):
            if nw * ns <= nblk:
                plans.add((ns, nw, -(-nblk // (nw * ns))))
    same_n = kcap - 40
    saved = ops.ATTN_PIPE
    try:
        for plan in sorted(plans):
            ns = plan[0]
            po = torch.empty(B * nkv * ns * 16 * hd, device="cuda")
            pml = torch.empty(B * nkv * ns * 16 * 2, device="cuda")
            kw = dict(B=B, Lkv=0, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, kcap=kcap, part_o=po, part_ml=pml,
                      counters=cnt, plan=plan)
            o = torch.full((B, nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
            q8ok = ops.attn_decode_q8_ok(nh, nkv, hd, plan[1])
            q8 = torch.full((B, nh * hd), 0x55, dtype=torch.uint8, device="cuda")
            q8s = torch.zeros(B, device="cuda")
            for rep in range(3):
                ops.ATTN_PIPE = rep != 2
                ops.attn_decode(q, nh * hd, o, nh * hd, kd, vd, lkv_dev=rows, rows=True,
                                q8=q8 if rep == 1 and q8ok else None, q8_scale=q8s if rep == 1 and q8ok else None, **kw)
                torch.cuda.synchronize()
                assert int(cnt.abs().sum()) == 0, plan
                if rep == 0:
                    first = o.clone()
                assert torch.equal(first, o), (plan, rep)
            if q8ok:
                r8, rs = ops.quant_fp8(o)
                assert torch.equal(q8, r8) and torch.equal(q8s, rs), plan
            assert err(o, ref) < KTOL, (plan, lens)
            ops.ATTN_PIPE = saved
            a, b2 = torch.empty_like(o), torch.empty_like(o)
            ops.attn_decode(q, nh * hd, a, nh * hd, kd, vd, lkv_dev=i32([same_n]), **kw)
            ops.attn_decode(q, nh * hd, b2, nh * hd, kd, vd, lkv_dev=i32([same_n] * B), rows=True, **kw)
            torch.cuda.synchronize()
            assert torch.equal(a, b2) and int(cnt.abs().sum()) == 0, plan
    finally:
        ops.ATTN_PIPE = saved


# ---------------------------------------------------------------------------------- 3. KV append, merge prologue
def _qkv_setup(M, H, nh, nkv, hd, Smax, seed=60):
    from pghip import engine
    from pghip.weights import rope_row_perm
    nblk = nh + 2 * nkv
    W = rnd(nblk * hd, H, scale=1 / 22, seed=seed)
    Wp = W.view(nblk, hd, H)[:, rope_row_perm(hd).cuda(), :].reshape(nblk * hd, H).contiguous()
    x = rnd(M, H, seed=seed + 1)
    cos_t, sin_t = engine.rope_tables(hd, 1024, 10000.0, "cuda")
    return Wp, x, cos_t, sin_t


def _caches(B, Smax, kvd, seed):
    """(kc, vtc, kd, vd) filled with one finite random pattern: an untouched slot keeps it."""
    kc = rnd(B, Smax, kvd, seed=seed)
    vtc = rnd(B, kvd, Smax, seed=seed + 1)
    kd = rnd(B * Smax * kvd, seed=seed + 2)
    vd = rnd(B * Smax * kvd, seed=seed + 3)
    return kc, vtc, kd, vd


@pytest.mark.parametrize("M,H,nh,nkv,hd,frag", [(2, 512, 8, 1, 256, False), (3, 512, 8, 1, 256, True),
                                                 (8, 128, 4, 2, 32, True), (16, 512, 8, 1, 256, False),
                                                 (17, 512, 8, 1, 256, False),      # tile GEMM, fused epilogue
                                                 (20, 2048, 8, 1, 256, False)])    # split K + pg_gemm_finalize
def test_qkv_rope_append_per_row_slots(M, H, nh, nkv, hd, frag):
    """PG_EPI_QKV_ROPE with PG_SLOT_ROWS: row b's k / v land at slot slot_dev[b] + slot_base in all four cache layouts
    (kc, vtc and the decode-order kd, vd) and no other slot changes.  Exact.  Up to 16 rows (the GEMV): against the
    same launch of row b alone at B = 1 with the shared slot word.  Above (the tile GEMM and pg_gemm_finalize, whose
    one-row form would be another kernel): against the whole batch launched with the shared word slot_dev[b], of
    which row b's cache is kept."""
    from pghip import ops
    from pghip.weights import frag_pack
    Smax, kvd = 192, nkv * hd
    Wp, x, cos_t, sin_t = _qkv_setup(M, H, nh, nkv, hd, Smax)
    Wk = frag_pack(Wp) if frag else Wp
    flag = ops.W_FRAG if frag else 0
    slots = [(5 + 37 * b) % (Smax - 3) + 1 for b in range(M)]            # slot_dev values; slot = value - 1
    slots[0], slots[-1] = 19, Smax                                       # ... one at the last slot of the cache
    pos = i32([s + 3 for s in slots])
    sd = i32(slots)
    c0 = _caches(M, Smax, kvd, 70)
    got = [t.clone() for t in c0]
    common = dict(head_dim=hd, cos_t=cos_t, sin_t=sin_t, smax=Smax, q_heads=nh, kv_heads=nkv, rows_per_batch=1)
    qg = torch.empty(M, nh * hd, dtype=torch.bfloat16, device="cuda")
    fa = ops.fused_args(pos=pos, slot_dev=sd, slot_base=-1, kc=got[0], vtc=got[1], kd=got[2], vd=got[3], **common)
    ops.gemm_fused(x, Wk, qg, fa, epi=ops.EPI_QKV_ROPE | flag | ops.SLOT_ROWS, M=M)
    want = [t.clone() for t in c0]
    qw = torch.empty_like(qg)
    per = Smax * kvd
    for b in range(M):
        if M <= 16:
            w1 = [want[0][b], want[1][b], want[2][b * per:(b + 1) * per], want[3][b * per:(b + 1) * per]]
            fa = ops.fused_args(pos=pos[b:b + 1], slot_dev=sd[b:b + 1], slot_base=-1, kc=w1[0], vtc=w1[1], kd=w1[2],
                                vd=w1[3], **common)
            ops.gemm_fused(x[b:b + 1], Wk, qw[b:b + 1], fa, epi=ops.EPI_QKV_ROPE | flag, M=1)
        else:
            tmp = [t.clone() for t in c0]
            qt = torch.empty_like(qg)
            fa = ops.fused_args(pos=pos, slot_dev=sd[b:b + 1], slot_base=-1, kc=tmp[0], vtc=tmp[1], kd=tmp[2],
                                vd=tmp[3], **common)
            ops.gemm_fused(x, Wk, qt, fa, epi=ops.EPI_QKV_ROPE | flag, M=M)
            want[0][b], want[1][b] = tmp[0][b], tmp[1][b]
            want[2][b * per:(b + 1) * per] = tmp[2][b * per:(b + 1) * per]
            want[3][b * per:(b + 1) * per] = tmp[3][b * per:(b + 1) * per]
            qw[b] = qt[b]
    torch.cuda.synchronize()
    assert torch.equal(qg, qw)
    for name, g_, w_ in zip(("kc", "vtc", "kd", "vd"), got, want):
        assert torch.equal(g_, w_), name
    # ... and only slot slot_dev[b] - 1 of row b changed, in the canonical layouts (kd / vd are permutations of them)
    for b in range(M):
        keep = torch.ones(Smax, dtype=torch.bool, device="cuda")
        keep[slots[b] - 1] = False
        assert torch.equal(got[0][b][keep], c0[0][b][keep]) and torch.equal(got[1][b][:, keep], c0[1][b][:, keep]), b
        assert not torch.equal(got[0][b][~keep], c0[0][b][~keep]), b
    kd_r, vd_r = ops.decode_cache_pack(got[0], got[1], nkv)
    ch = torch.zeros(M, Smax, dtype=torch.bool, device="cuda")
    ch[torch.arange(M), torch.tensor(slots) - 1] = True
    chd, _ = ops.decode_cache_pack(ch[:, :, None].expand(M, Smax, kvd).contiguous().to(torch.bfloat16),
                                   ch[:, None, :].expand(M, kvd, Smax).contiguous().to(torch.bfloat16), nkv)
    chd = chd.reshape(-1) != 0
    assert torch.equal(got[2][chd], kd_r.reshape(-1)[chd]) and torch.equal(got[2][~chd], c0[2][~chd])


@pytest.mark.parametrize("B,z", [(2, 1), (2, 2), (1, 2)])
def test_attention_merge_prologue_per_row_split_count(B, z):
    """pro_mode 2 (the o_proj GEMV that merges the split-KV partials) with PG_SLOT_ROWS and more than 16 splits -- the
    form that reads the kv length to skip the empty splits: row m merges its own ceil((slot_dev[m] + slot_base + 1) /
    akeys) splits.  The partials past each row's count are overwritten with finite garbage that a shared count (the
    longest row's) would merge.  Exact against the same launch of each row alone with the shared word."""
    from pghip import ops
    nh, nkv, hd, kcap, SK = 8, 1, 256, 640, 32
    kvd, nsplit, dt = nkv * hd, 20, 256
    lens = [600, 19][:B] if B > 1 else [70]                 # keys each row attends, its new token included
    q = rnd(B, nh * hd, seed=81)
    kc, vtc = rnd(B, kcap, kvd, seed=82), rnd(B, kvd, kcap, seed=83)
    kd, vd = ops.decode_cache_pack(kc, vtc, nkv)
    po = torch.empty(B * nkv * nsplit * 16 * dt, device="cuda")
    pml = torch.empty(B * nkv * nsplit * 16 * 2, device="cuda")
    pos = i32(lens)                                          # position = keys once the token is appended
    ops.attention_rows(q, nh * hd, None, nh * hd, kc, kcap * kvd, hd, kvd, vtc, kvd * kcap, hd * kcap, kcap,
                       B=B, Lq=1, Lkv=0, lkv_rows=pos, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, split_keys=SK,
                       nsplit=nsplit, part_o=po, part_ml=pml, kcap=kcap, kd=kd, vd=vd)
    ref_o = torch.empty(B, nh * hd, dtype=torch.bfloat16, device="cuda")
    ops.attn_combine(po, pml, ref_o, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=nsplit)
    pov, pmlv = po.view(B, nkv, nsplit, 16, dt), pml.view(B, nkv, nsplit, 16, 2)
    for b, n in enumerate(lens):                            # garbage where the row has no keys
        used = -(-n // SK)
        pov[b, :, used:] = 3.0
        pmlv[b, :, used:, :, 0] = 4.0
        pmlv[b, :, used:, :, 1] = 2.0
    Wo = rnd(2048, nh * hd, scale=1 / 45, seed=84)
    kw = dict(pro_mode=ops.PRO_ATTN_COMBINE, asplit=nsplit, head_dim=hd, dtw=dt, q_per_kv=nh // nkv, kv_heads=nkv,
              akeys=SK)
    got = torch.empty(z, B, 2048, device="cuda")
    fa = ops.fused_args(part_o=po, part_ml=pml, slot_dev=pos, slot_base=-1, **kw)
    ops.gemm_fused(None, Wo, got, fa, epi=ops.EPI_F32 | ops.SLOT_ROWS, M=B, ksplit=z)
    for b in range(B):
        one = torch.empty(z, 1, 2048, device="cuda")
        fa = ops.fused_args(part_o=pov[b], part_ml=pmlv[b], slot_dev=i32([lens[b] - 1]), slot_base=0, **kw)
        ops.gemm_fused(None, Wo, one, fa, epi=ops.EPI_F32, M=1, ksplit=z)
        assert torch.equal(got[:, b], one[:, 0]), b
    assert err(got.sum(0), ref_o.float() @ Wo.float().t()) < 1e-2


# ------------------------------------------------------------------------------------------------------- 4. engine
@pytest.fixture(scope="module")
def tiny():
    from pghip import configs, engine, synthetic, weights
    cfg = configs.TINY
    return engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__))


@pytest.fixture(scope="module")
def tiny_fp8():
    from pghip import configs, engine, synthetic, weights
    cfg = configs.TINY
    return engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__,
                                                             fp8=True))


def nerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _teacher_forced(eng, B):
    """Prefill + teacher-forced decode logits of the ragged batch of the first B pool requests: [STEPS][B][V] and the
    ids the engine picked, each row fed its own oracle continuation."""
    ids, mask, px, lens = R.batch(B)
    refs = [R.reference(b) for b in range(B)]
    cache, feats, logits, nxt = eng.prefill_request(torch.from_numpy(ids).cuda(), torch.from_numpy(px).cuda(),
                                                    torch.from_numpy(mask).cuda(), R.STEPS)
    assert cache.ragged and nxt.tolist() == [n + 1 for n in lens]
    st = eng.decode_state(B, cache, nxt, R.STEPS)
    assert st["ragged"]
    out, picked = [logits.cpu().numpy()], [logits.argmax(-1).cpu().numpy()]
    for t in range(1, R.STEPS):
        st["ids"].copy_(torch.tensor([refs[b][0][t - 1] for b in range(B)], device="cuda"))      # teacher forcing
        lg = eng.decode_step(st, cache, feats, dict(do_sample=False))
        out.append(lg.cpu().numpy().copy())
        picked.append(st["ids"].cpu().numpy().copy())
    assert st["pos"].tolist() == [n + R.STEPS for n in lens]
    return np.stack(out), np.stack(picked), refs


@pytest.mark.parametrize("B,fuse_max_b,use_fin,fused_rounds", [(2, 2, True, 2), (2, 2, False, 2), (2, 0, True, 2),
                                                                (3, 2, True, 2), (3, 2, True, 1),
                                                                (8, 2, True, 2), (8, 2, True, 1), (8, 2, False, 2)])
def test_ragged_prefill_and_teacher_forced_decode_vs_oracle(tiny, B, fuse_max_b, use_fin, fused_rounds):
    """Every row of a ragged batch against oracle.generate run on that row alone, unpadded: prefill logits and 15
    teacher-forced decode steps within TOL, ids equal where the oracle's margin exceeds 0.1.  The layer forms as in
    test_tiny_teacher_forced_decode_vs_oracle: B = 2 with the merge in the o_proj prologue (finalised in-kernel, and
    the split-K-partials form), the unfused layer (fuse_max_b = 0, and B = 3), 5..16 rows finalised in-kernel (B = 8)
    and unfused; fused_rounds = 1 sends B > 2 through the one-launch attention (pg_attn_decode_rows) on this short
    cache."""
    eng = tiny
    eng.FUSE_MAX_B, eng.USE_FIN, eng.FUSED_MIN_ROUNDS = fuse_max_b, use_fin, fused_rounds
    try:
        got, picked, refs = _teacher_forced(eng, B)
    finally:
        eng.FUSE_MAX_B, eng.USE_FIN = type(eng).FUSE_MAX_B, type(eng).USE_FIN
        eng.FUSED_MIN_ROUNDS = type(eng).FUSED_MIN_ROUNDS
    worst = 0.0
    for b in range(B):
        ref_ids, ref_logits, margin = refs[b]
        for t in range(R.STEPS):
            e = nerr(got[t][b:b + 1], ref_logits[t])
            worst = max(worst, e)
            assert e < TOL, (b, t, e)
            if margin[t] > R.MARGIN:
                assert int(picked[t][b]) == ref_ids[t], (b, t)
    print(f"ragged B={B} fuse_max_b={fuse_max_b} use_fin={use_fin}: worst scaled logit error {worst:.4f}")


def test_ragged_fp8_batch_17_vs_oracle(tiny_fp8):
    """fp8 engine, 17 ragged rows (every Gemma linear on e4m3 operands: the prefill tiles and the 17..32-row GEMVs, the
    one-launch attention writing the fp8 row copy): each row against the fp32 oracle on that row alone.  Bound: 1.5x
    the distance of the oracle run on the same operand rounding (bf16_operands + fp8_operands(min_rows=0), computed
    here per row and step, the largest taken -- the rule of the tensor-parallel fp8 decode check); ids equal where the
    oracle's margin exceeds 0.1 and twice that bound in logit units."""
    from oracle import paligemma_oracle as O
    eng = tiny_fp8
    B = 17
    fe, ie, amax = [], [], 0.0
    runs = {}
    for rounds in (2, 1):
        eng.FUSED_MIN_ROUNDS = rounds
        try:
            runs[rounds] = _teacher_forced(eng, B)
        finally:
            eng.FUSED_MIN_ROUNDS = type(eng).FUSED_MIN_ROUNDS
    refs = runs[2][2]
    lm8 = getattr(eng.w, "lm_w8f", None) is not None
    emu = []
    for b in range(B):
        ids, px = R.request(b)
        with O.bf16_operands(), O.fp8_operands(min_rows=0, lm_head=lm8):
            _, lg = O.generate(R.oracle(), ids, px, np.ones_like(ids), R.STEPS, stop_token=None, teacher=refs[b][0],
                               record_logits=True)
        emu.append(lg)
        for t in range(R.STEPS):
            ie.append(nerr(lg[t], refs[b][1][t]))
            amax = max(amax, float(np.abs(refs[b][1][t]).max()))
    bound = 1.5 * max(ie)
    for rounds, (got, picked, _) in runs.items():
        for b in range(B):
            for t in range(R.STEPS):
                e = nerr(got[t][b:b + 1], refs[b][1][t])
                fe.append(e)
                assert e < bound, (rounds, b, t, e, bound)
                if refs[b][2][t] > max(R.MARGIN, 2 * bound * amax):
                    assert int(picked[t][b]) == refs[b][0][t], (rounds, b, t)
    print(f"ragged fp8 B=17: worst scaled logit error {max(fe):.4f}, emulated oracle {max(ie):.4f}")


# ----------------------------------------------------------------------------------------------------- 5. generate
_SINGLE = {}
# The decode layers take one of three forms by batch size (engine._decode_route), equal to the oracle within TOL but not
# to one another bit for bit (test_tiny_batched_decode_fin_path_vs_oracle bounds two of them at 5e-3 of the logits'
# scale, 0.012 logits, and TINY's top-1 margins fall below that at about one step in ten).  The row alone at B = 1 is
# therefore run on the form its batch takes, so that what the comparison sees is the batching, not the form:
#   B = 2  the B <= 2 form, which B = 1 takes anyway
#   B = 3  the unfused layer: FUSE_MAX_B = 0 sends B = 1 there too
#   B = 8  5..16 rows finalised in-kernel: FIN_MIN_B = 1 with FUSE_MAX_B = 0
FORM = {2: {}, 3: dict(FUSE_MAX_B=0), 8: dict(FUSE_MAX_B=0, FIN_MIN_B=1)}


def _single(eng, b, B=2):
    """Free-running greedy ids of pool request b alone, unpadded, at B = 1, on the layer form a batch of B takes
    (computed once per form)."""
    key = (b, tuple(sorted(FORM[B].items())))
    if key not in _SINGLE:
        ids, px = R.request(b)
        t = torch.from_numpy(ids).cuda()
        for k, v in FORM[B].items():
            setattr(eng, k, v)
        try:
            _SINGLE[key] = eng.generate(t, torch.from_numpy(px).cuda(), torch.ones_like(t), R.STEPS, stop_token=None,
                                        use_graph=True)[0].tolist()
        finally:
            for k in FORM[B]:
                setattr(eng, k, getattr(type(eng), k))
    return _SINGLE[key]


def _check_rows(got, want, rows, what):
    """Every row's ids equal.  A row may differ only by a sub-margin tie -- its first differing step is one where the
    oracle (which the B = 1 run followed so far) has a top-1 margin below 0.1 -- and at most one row of the batch."""
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    for i in bad:
        t = next(k for k in range(len(want[i])) if got[i][k] != want[i][k])
        ref_ids, _, margin = R.reference(rows[i])
        assert want[i][:t] == list(ref_ids[:t]) and margin[t] < R.MARGIN, (what, rows[i], t, got[i], want[i])
    assert len(bad) <= 1, (what, bad, [(got[i], want[i]) for i in bad])


@pytest.mark.parametrize("B", [2, 3, 8])
def test_ragged_generate_equals_each_row_alone(tiny, B):
    """Free-running greedy ids of each row of a ragged batch == generate on that row alone at B = 1: hipGraph and eager
    steps, chained (pg_argmax_embed) and unchained; the row alone runs on the layer form its batch takes (FORM).  The
    requests' seeds keep the oracle's margin above 0.04 at every step (ragged_ref.SEEDS) but not above 0.1, so no row
    is excluded up front: a row is excused only where it actually differs, at a step whose oracle margin is below 0.1
    (_check_rows), and at most one per batch.  On the tree before per-row lengths the short rows' first token came from
    a pad position and this fails."""
    eng = tiny
    ids, mask, px, lens = R.batch(B)
    want = [_single(eng, b, B) for b in range(B)]
    t_ids, t_mask, t_px = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(px).cuda()
    try:
        for chain in (True, False):
            eng.CHAIN_EMBED = chain
            for use_graph in (True, False):
                got = eng.generate(t_ids, t_px, t_mask, R.STEPS, stop_token=None, use_graph=use_graph).tolist()
                _check_rows(got, want, list(range(B)), (chain, use_graph))
    finally:
        eng.CHAIN_EMBED = type(eng).CHAIN_EMBED


def test_ragged_generate_per_row_eos_and_uniform_padding(tiny):
    """Per-row EOS trimming with return_list=True on a ragged batch (the stop token is one that rows reach at different
    steps, or never), the padded [B][n] form, and a uniformly padded batch -- every row the same length, five pad
    columns, so the per-row path runs with equal lengths -- equal to the all-ones call on the unpadded ids."""
    eng = tiny
    B = 3
    ids, mask, px, lens = R.batch(B)
    want = [_single(eng, b, B) for b in range(B)]
    stop = want[0][3]
    cut = [w[: w.index(stop) + 1] if stop in w else w for w in want]
    t_ids, t_mask, t_px = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(px).cuda()
    rows = eng.generate(t_ids, t_px, t_mask, R.STEPS, stop_token=stop, return_list=True)
    _check_rows(rows, cut, list(range(B)), "eos list")
    out = eng.generate(t_ids, t_px, t_mask, R.STEPS, stop_token=stop, pad_token=0)
    for b in range(B):
        if rows[b] == cut[b]:
            assert out[b, : len(cut[b])].tolist() == cut[b] and (out[b, len(cut[b]):] == 0).all()
    # uniform: rows 4 and 5 cut to 64 tokens each, then padded to 69
    u_ids = np.stack([R.request(4)[0][0], R.request(5)[0][0, :64]])
    u_px = np.concatenate([R.request(4)[1], R.request(5)[1]])
    plain = eng.generate(torch.from_numpy(u_ids).cuda(), torch.from_numpy(u_px).cuda(),
                         torch.ones(2, 64, dtype=torch.int64).cuda(), R.STEPS, stop_token=None).tolist()
    p_ids = np.concatenate([u_ids, np.zeros((2, 5), np.int64)], 1)
    p_mask = np.concatenate([np.ones((2, 64), np.int64), np.zeros((2, 5), np.int64)], 1)
    padded = eng.generate(torch.from_numpy(p_ids).cuda(), torch.from_numpy(u_px).cuda(),
                          torch.from_numpy(p_mask).cuda(), R.STEPS, stop_token=None).tolist()
    assert padded == plain


def test_all_ones_mask_takes_the_shared_length_path(tiny):
    """An all-ones mask leaves the cache and the decode state on the shared-length path (one kv_len word, no per-row
    launches), and a mask that is not right-padded raises before anything is launched."""
    eng = tiny
    ids, px = R.request(4)
    t = torch.from_numpy(np.repeat(ids, 2, 0)).cuda()
    p = torch.from_numpy(np.repeat(px, 2, 0)).cuda()
    cache, feats, logits, nxt = eng.prefill_request(t, p, torch.ones_like(t), 4)
    st = eng.decode_state(2, cache, nxt, 4)
    assert not cache.ragged and not st["ragged"] and int(st["kv_len"]) == t.shape[1]
    bad = torch.ones_like(t)
    bad[1, :2] = 0
    with pytest.raises(ValueError, match="right-padded"):
        eng.generate(t, p, bad, 4)
