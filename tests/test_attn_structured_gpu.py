"""Attention kernels on structured inputs (tests/attn_ref.py): census, needle, ramp up / down and spike through every
attention entry point and kernel form, against fp64 softmax attention computed on the device.

Bounds (attn_ref): census |o - count_d / L| <= 2^-7 count_d / L; everything else |o - ref| <= C budget + 1e-30 per
element with budget = softmax @ |v| and C = 2^-6 from the CPU emulation.  Each case prints its worst ratio (in units of
the bound's own scale: count_d / L for census, budget otherwise).

The form a shape reaches is decided by attn_form (csrc/attn.hip); the arithmetic stands beside each shape.  Shapes are
(B, L, nh, nkv, hd), rows = L nh / nkv stacked query rows per kv head, wgs(r) = ceil(rows / r) nkv B, rounds(r) =
ceil(wgs(r) / 256).
"""
import pytest
import torch

import attn_ref as R
from test_ragged_gpu import _decode_lens, ragged_lens

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------ inputs and checks
def _last_block_key(n):
    """A key inside the last 32-key block of n keys."""
    return n - 1 - ((n - 1) % 32) // 2


def _cases(B, nh, nkv, Lq, D, Smax, lens, spikes, fills=None, names=None):
    """(name, q, k, v, ref, unit, c) per structured input, built and referenced once, on the device: the caller runs
    every variant of its entry point on the same tensors.  spikes: {tag: [B] key per row}; fills (decode): the needle
    lists of attn_ref.edge_fills.  ref / unit broadcast against o [B][nh][Lq][D]; the bound is c * unit + 1e-30."""
    a = (B, nh, nkv, Lq, D, Smax, lens)
    built = [("census", lambda: R.census(*a, seed=11, device="cuda"))]
    if fills is None:
        built.append(("needle", lambda: R.needle(*a, seed=12, device="cuda")))
    else:
        for f, nd in enumerate(fills):
            built.append((f"needle{f}", lambda nd=nd, f=f: R.needle(*a, seed=12 + 100 * f, needles=nd, device="cuda")))
    built.append(("ramp_up", lambda: R.ramp(*a, seed=13, device="cuda")))
    built.append(("ramp_down", lambda: R.ramp(*a, seed=14, down=True, device="cuda")))
    for tag, sp in spikes.items():
        built.append((f"spike_{tag}", lambda sp=sp: R.ramp(*a, seed=15, down=True, spike=sp, device="cuda")))
    for name, make in built:
        if names is not None and not any(name.startswith(n) for n in names):
            continue
        q, k, v = make()
        if name == "census":
            ref = torch.stack([R.census_expected(D, n) for n in lens]).cuda()[:, None, None, :]
            yield name, q, k, v, ref, ref, R.CENSUS_RTOL
        else:
            ref, budget = R.ref(q, k, v, D ** -0.5, lens=lens)
            yield name, q, k, v, ref, budget, R.C


def _check(tag, name, o, ref, unit, c, nrows=None):
    """o [B][nh][Lq][D] against ref within c * unit + 1e-30 (query rows below nrows[b] only); prints the worst ratio."""
    assert torch.isfinite(o.float()).all(), (tag, name)
    d = (o.double() - ref).abs()
    bad = d > c * unit + 1e-30
    ratio = torch.where(unit > 0, d / unit.clamp_min(1e-300), torch.where(d > 0, float("inf"), 0.0).double())
    if nrows is not None:
        keep = (torch.arange(o.shape[2], device="cuda")[None, :] < i32(nrows)[:, None])[:, None, :, None]
        bad, ratio = bad & keep, torch.where(keep, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max())
    print(f"{tag} {name}: worst ratio {worst * 256:.3f} * 2^-8 (bound {c * 256:g} * 2^-8)")
    assert not bool(bad.any()), (tag, name, worst)
    return worst


def _layout(q, k, v):
    """The cache layout of the entry points: q [B*Lq][nh*D], k [B][Smax][nkv*D], V^T [B][nkv*D][Smax], bf16."""
    B, nh, Lq, D = q.shape
    nkv, Smax = k.shape[1], k.shape[2]
    qf = q.permute(0, 2, 1, 3).reshape(B * Lq, nh * D).to(BF).contiguous()
    kc = k.permute(0, 2, 1, 3).reshape(B, Smax, nkv * D).to(BF).contiguous()
    vtc = v.permute(0, 1, 3, 2).reshape(B, nkv * D, Smax).to(BF).contiguous()
    return qf, kc, vtc


def _heads(o, B, Lq, nh, D):
    return o.view(B, Lq, nh, D).permute(0, 2, 1, 3)


def _smax(L):
    return (L + 8 + 63) // 64 * 64          # V^T rows readable up to the next 32-key block, 16-B aligned strides


# --------------------------------------------------------------------------------------------------------- prefill
# (B, L, nh, nkv, hd, nks, masked)
FLASH4 = [(1, 264, 8, 1, 256, 0, False),    # rows 2112: wgs(128) = 17 < 256 -> 4 waves
          (2, 100, 4, 4, 72, 0, False),     # rows 100: wgs(128) = 1 * 4 * 2 = 8
          (2, 70, 4, 2, 24, 0, False),      # rows 140: wgs(128) = 2 * 2 * 2 = 8; head_dim 24 in the 32-wide instance
          (2, 150, 8, 2, 128, 0, False)]    # rows 600: wgs(128) = 5 * 2 * 2 = 20
FLASH8_72 = [(16, 250, 16, 16, 72, 0, False)]   # rows 250: wgs(128) = 2 * 16 * 16 = 512 >= 256 -> 8 waves (DP 96)
FLASH8_256 = [(32, 125, 8, 1, 256, 0, False)]   # rows 1000: wgs(256) = 4 * 32 = 128 < 256, so no 8 x 32; wgs(128) =
#                                                 8 * 32 = 256 -> 8 waves; wgs(192) = 6 * 32 = 192: 1 round * 12 is not
#                                                 < 1 round * 8, so 12 waves do not win
FLASH12 = [(14, 300, 8, 1, 256, 0, False)]      # rows 2400: wgs(256) = 140 < 256; wgs(128) = 19 * 14 = 266 -> 8 waves,
#                                                 2 rounds * 8 = 16; wgs(192) = 13 * 14 = 182: 1 round * 12 = 12 < 16
FLASH8X32 = [(32, 250, 8, 1, 256, 0, False)]    # rows 2000: wgs(256) = 8 * 32 = 256 >= 256, rounds(256) = 1;
#                                                 rounds(128) = ceil(512 / 256) = 2, rounds(192) = ceil(352 / 256) = 2:
#                                                 1 * 25 < 2 * 16 and 1 * 25 < 2 * 24 -> 8 waves x 32 rows, 32-key blocks
KEYSPLIT = [(1, 264, 8, 1, 256, 5, False),      # 4 waves, 64-key blocks: 5 blocks, one per split
            (1, 100, 8, 1, 256, 5, False),      # 2 blocks in 5 splits: splits 2..4 left empty
            (1, 256, 16, 16, 72, 4, False)]     # 4 blocks, one per split
ONEWAVE = [(2, 100, 4, 2, 64, 0, True),         # an additive mask keeps pg_attention off the flash kernel; 16-row groups
           (1, 70, 8, 1, 256, 0, True),         # wgs16 = ceil(rows / 16) nkv B = 13 * 2 * 2 = 52, 35, 4 * 4 * 2 = 32,
           (2, 50, 4, 4, 72, 0, True)]          # all < 1024 -> the one-wave attn_kernel
LDS = [(8, 130, 16, 1, 32, 0, True),            # rows 2080: wgs16 = 130 * 8 = 1040 >= 1024 -> attn_lds_kernel
       (8, 260, 8, 1, 256, 0, True)]            # rows 2080: 1040


def _split_first_key(n, nks):
    """First key of the last non-empty key split of n keys (attn_fa_kernel: ceil(n / 64) blocks, ceil(blocks / nks)
    per split); unsplit, that is the first block."""
    if nks <= 1:
        return 0
    nblk = -(-n // 64)
    per = -(-nblk // nks)
    return (nblk - 1) // per * per * 64


def _prefill(shape, ragged, names=None):
    from pghip import ops
    B, L, nh, nkv, hd, nks, masked = shape
    Smax = _smax(L)
    kvd = nkv * hd
    # (ragged_lens wants the longest row two 64-key blocks past the 19-key row; for a shorter L its lengths for 147
    # keys are clamped to L -- the same short, block-edge and full rows)
    lens = [min(x, L) for x in ragged_lens(B, max(L, 147))] if ragged else [L] * B
    spikes = {"last": [_last_block_key(n) for n in lens],
              "first": [min(_split_first_key(n, nks) + 3, n - 1) for n in lens]}
    tag = f"prefill{'_rows' if ragged else ''} {shape}"
    kw = dict(B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5)
    if nks:
        no, nml = ops.prefill_split_workspace(B, L, nh, nkv, hd, nks)
        kw.update(nsplit=nks, part_o=torch.full((no,), float("nan"), device="cuda"),
                  part_ml=torch.full((nml,), float("nan"), device="cuda"))
    if masked:
        kw.update(mask=torch.zeros(B, L, L, device="cuda"), mask_bs=L * L, mask_rs=L)
    for name, q, k, v, ref, unit, c in _cases(B, nh, nkv, L, hd, Smax, lens, spikes, names=names):
        qf, kc, vtc = _layout(q, k, v)
        o = torch.full((B * L, nh * hd), float("nan"), dtype=BF, device="cuda")
        args = (qf, nh * hd, o, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax)
        if ragged:
            ops.attention_rows(*args, lkv_rows=i32(lens), **kw)
        else:
            ops.attention(*args, **kw)
        _check(tag, name, _heads(o, B, L, nh, hd), ref, unit, c, nrows=lens if ragged else None)


def _ids(shapes):
    return ["x".join(str(int(x)) for x in s) for s in shapes]


_SHARED = FLASH4 + FLASH8_72 + FLASH8_256 + FLASH12 + FLASH8X32 + KEYSPLIT + ONEWAVE + LDS
_RAGGED = FLASH4 + FLASH8X32 + KEYSPLIT + ONEWAVE + LDS


@pytest.mark.parametrize("shape", _SHARED, ids=_ids(_SHARED))
def test_prefill_shared_length(shape):
    """pg_attention, Lq = Lkv = L: the 4- / 8- / 12-wave flash forms, 8 waves x 32 rows on 32-key blocks, key splits
    with attn_pf_combine_kernel, and under an all-zero additive mask the one-wave and the LDS-staged kernels."""
    _prefill(shape, ragged=False)


@pytest.mark.parametrize("shape", _RAGGED, ids=_ids(_RAGGED))
def test_prefill_per_row_lengths(shape):
    """pg_attention_rows: census, needle, ramp and spike built over each row's own length; query rows below it compared."""
    _prefill(shape, ragged=True)


# --------------------------------------------------------------------------------------- decode splits + pg_attn_combine
SPLIT_KEYS = (32, 64, 128, 256)
# (B, L, nh, nkv, hd, Smax): with kcap = Smax head_dim 256 takes attn_decode_wg_kernel<2> at 64-key splits and <4> at
# 128 / 256, attn_decode_kernel<true> at 32; head_dim 32 attn_decode_kernel<true>; head_dim 72 (D != DP) and every
# kcap = 0 call attn_decode_kernel<false>
DECODE = [(3, 200, 8, 1, 256, 256), (5, 300, 8, 2, 256, 448), (4, 40, 4, 1, 32, 64), (3, 100, 4, 1, 72, 128)]


def _split_edges(lens, ranges):
    """0, 31, 32, 63, 64, L - 2, L - 1 and the first and last key of every split (ranges: (first, last + 1) keys)."""
    edges = {0, 31, 32, 63, 64}
    for n in set(lens):
        edges |= {n - 2, n - 1}
    for lo, hi in ranges:
        edges |= {lo, hi - 1}
    top = max(lens)
    return sorted(e for e in edges if 0 <= e < top)


def _decode_split(shape, ragged, split_keys=SPLIT_KEYS, names=None):
    from pghip import ops
    B, L, nh, nkv, hd, Smax = shape
    kvd = nkv * hd
    lens = _decode_lens(B, Smax) if ragged else [L] * B
    ranges = [(s * sk, (s + 1) * sk) for sk in split_keys for s in range(-(-Smax // sk))]
    fills = R.edge_fills(_split_edges(lens, ranges), B, nkv, lens)
    spikes = {"last": [_last_block_key(n) for n in lens]}
    for sk in split_keys:                             # the first block of the last non-empty split of sk keys
        sp = [(n - 1) // sk * sk for n in lens]
        if sp not in spikes.values():
            spikes[f"first{sk}"] = sp
    tag = f"decode_split{'_rows' if ragged else ''} {shape}"
    dt = (hd + 15) // 16 * 16
    packed = hd % 32 == 0
    for name, q, k, v, ref, unit, c in _cases(B, nh, nkv, 1, hd, Smax, lens, spikes, fills, names=names):
        qf, kc, vtc = _layout(q, k, v)
        kd, vd = ops.decode_cache_pack(kc, vtc, nkv) if packed else (None, None)
        args = (qf, nh * hd, None, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax)
        worst = 0.0
        for sk in split_keys:
            ns = ((Smax + sk - 1) // sk + 3) // 4 * 4
            po = torch.full((B * nkv * ns * 16 * dt,), float("nan"), device="cuda")
            pml = torch.full((B * nkv * ns * 16 * 2,), float("nan"), device="cuda")
            for cap in (0, Smax):
                kw = dict(B=B, Lq=1, Lkv=1, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, split_keys=sk, nsplit=ns,
                          part_o=po, part_ml=pml, kcap=cap, kd=kd if cap else None, vd=vd if cap else None)
                o = torch.full((B, nh * hd), float("nan"), dtype=BF, device="cuda")
                if ragged:
                    ops.attention_rows(*args, lkv_rows=i32([n - 1 for n in lens]), **kw)
                else:
                    ops.attention(*args, lkv_dev=i32([L - 1]), **kw)
                ops.attn_combine(po, pml, o, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=ns)
                worst = max(worst, _check(f"{tag} sk={sk} kcap={cap}", name, _heads(o, B, 1, nh, hd), ref, unit, c))
        print(f"{tag} {name}: worst ratio over the split sizes {worst * 256:.3f} * 2^-8")


@pytest.mark.parametrize("ragged", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("shape", DECODE, ids=_ids(DECODE))
def test_decode_splits_and_combine(shape, ragged):
    """pg_attention / pg_attention_rows in split mode + pg_attn_combine over 32- to 256-key splits, with and without the
    decode-order copies: every split's first and last key is some (row, kv head)'s needle."""
    _decode_split(shape, ragged)


# ------------------------------------------------------------------- every (DP, DT) instance the launcher selects
# head_dim -> (DP, DT) = (32 ceil(hd / 32), ceil(hd / 16)), the eight pairs of attention_impl's switch (csrc/attn.hip)
HEAD_DIMS = {16: (32, 1), 24: (32, 2), 40: (64, 3), 64: (64, 4), 72: (96, 5), 88: (96, 6), 128: (128, 8),
             256: (256, 16)}


@pytest.mark.parametrize("hd", list(HEAD_DIMS))
def test_every_head_dim_instance(hd):
    """Needle and ramps through each (DP, DT) instance: B 2, L 70, nh 4, nkv 2 is rows 140, wgs(128) = 2 * 2 * 2 = 8
    < 256 -> the 4-wave flash form; under an all-zero additive mask wgs16 = 9 * 2 * 2 = 36 < 1024 -> the one-wave
    kernel; 32-key decode splits with kcap = 0 (attn_decode_kernel<false>) and with kcap = Smax, which is
    attn_decode_kernel<true> where head_dim == DP (64, 128, 256) and the guarded kernel with its first block
    prefetched elsewhere.  The bound is C: tests/test_attn_ref_host.py holds the emulation to C / 2 at 16, 40 and 88."""
    assert HEAD_DIMS[hd] == ((hd + 31) // 32 * 32, (hd + 15) // 16)
    B, L, nh, nkv = 2, 70, 4, 2
    names = ("needle", "ramp")
    _prefill((B, L, nh, nkv, hd, 0, False), ragged=False, names=names)
    _prefill((B, L, nh, nkv, hd, 0, True), ragged=False, names=names)
    _decode_split((B, L, nh, nkv, hd, _smax(L)), ragged=False, split_keys=(32,), names=names)


# ---------------------------------------------------------------------------------------------------- fused decode
FUSED = [(3, 200, 8, 1, 256, 256), (5, 300, 8, 2, 256, 448), (4, 40, 4, 1, 32, 64), (8, 97, 8, 1, 256, 128)]


def _fused_plans(B, nkv, kcap):
    """The plans test_attn_decode_fused walks: the engine's, and 2 / 4 waves x 1 / 3 / 16 splits where they fit."""
    from pghip import ops
    nblk = kcap // 32
    plans = {ops.decode_plan(B, nkv, kcap)}
    for nw in (2, 4):
        for ns in (1, 3, 16):
            if nw * ns <= nblk:
                plans.add((ns, nw, -(-nblk // (nw * ns))))
    return sorted(plans)


@pytest.mark.parametrize("ragged", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("shape", FUSED, ids=_ids(FUSED))
def test_decode_fused(shape, ragged):
    """pg_attn_decode / pg_attn_decode_rows: every plan, staggered form on and off; split sp owns the 32-key blocks
    [sp nblk / S, (sp + 1) nblk / S), and each such range's first and last key is a needle.  Tickets zero after each
    call."""
    from pghip import ops
    B, L, nh, nkv, hd, kcap = shape
    lens = _decode_lens(B, kcap) if ragged else [L] * B
    plans = _fused_plans(B, nkv, kcap)
    nblk = kcap // 32
    ranges = [(32 * (sp * nblk // ns), 32 * ((sp + 1) * nblk // ns)) for ns, _, _ in plans for sp in range(ns)]
    fills = R.edge_fills(_split_edges(lens, ranges), B, nkv, lens)
    spikes = {"last": [_last_block_key(n) for n in lens]}
    for ns, _, _ in plans:                            # the first block of the last non-empty split of the plan
        starts = [32 * (s * nblk // ns) for s in range(ns)]
        sp = [max(x for x in starts if x < n) for n in lens]
        if sp not in spikes.values():
            spikes[f"first{ns}"] = sp
    tag = f"decode_fused{'_rows' if ragged else ''} {shape}"
    cnt = torch.zeros(B * nkv, dtype=torch.int32, device="cuda")
    saved = ops.ATTN_PIPE
    try:
        for name, q, k, v, ref, unit, c in _cases(B, nh, nkv, 1, hd, kcap, lens, spikes, fills):
            qf, kc, vtc = _layout(q, k, v)
            kd, vd = ops.decode_cache_pack(kc, vtc, nkv)
            worst = 0.0
            for plan in plans:
                ns = plan[0]
                po = torch.full((B * nkv * ns * 16 * hd,), float("nan"), device="cuda")
                pml = torch.full((B * nkv * ns * 16 * 2,), float("nan"), device="cuda")
                for pipe in (True, False):
                    ops.ATTN_PIPE = pipe
                    o = torch.full((B, nh * hd), float("nan"), dtype=BF, device="cuda")
                    lk = dict(lkv_dev=i32(lens), Lkv=0, rows=True) if ragged else dict(lkv_dev=i32([L - 1]), Lkv=1)
                    ops.attn_decode(qf, nh * hd, o, nh * hd, kd, vd, B=B, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5,
                                    kcap=kcap, part_o=po, part_ml=pml, counters=cnt, plan=plan, **lk)
                    torch.cuda.synchronize()
                    assert int(cnt.abs().sum()) == 0, (plan, pipe)
                    worst = max(worst, _check(f"{tag} plan={plan} pipe={int(pipe)}", name, _heads(o, B, 1, nh, hd),
                                              ref, unit, c))
            print(f"{tag} {name}: worst ratio over the plans {worst * 256:.3f} * 2^-8")
    finally:
        ops.ATTN_PIPE = saved


# ------------------------------------------------------------------------------- o_proj merge prologue, W = identity
@pytest.mark.parametrize("B", [1, 3])
def test_oproj_merge_prologue_against_the_reference(B):
    """PRO_ATTN_COMBINE against fp64 attention, not against pg_attn_combine: split-mode partials, then the o_proj GEMV
    with W the 2048 x 2048 identity and an fp32 epilogue, whose summed K slabs are the merged attention row as the
    prologue staged it.  Row-major and fragment-packed W, ksplit 1 and 2.  (At head_dim 256 a needle or a spike holds all
    of the weight to fp64 precision and the row is v[key] exactly; census and the ramps carry the merge's arithmetic.)"""
    from pghip import ops
    from pghip.weights import frag_pack
    nh, nkv, hd, L, Smax = 8, 1, 256, 200, 256
    kvd = nkv * hd
    SK, nsplit, dt = 32, 8, 256
    lens = [L] * B
    ranges = [(s * SK, (s + 1) * SK) for s in range(nsplit)]
    fills = R.edge_fills(_split_edges(lens, ranges), B, nkv, lens)
    spikes = {"last": [_last_block_key(L)] * B, "first": [(L - 1) // SK * SK] * B}
    eye = torch.eye(nh * hd, dtype=BF, device="cuda")
    forms = [(eye, 0, "row-major"), (frag_pack(eye), ops.W_FRAG, "frag")]
    for name, q, k, v, ref, unit, c in _cases(B, nh, nkv, 1, hd, Smax, lens, spikes, fills,
                                              names=("census", "needle", "ramp", "spike")):
        qf, kc, vtc = _layout(q, k, v)
        po = torch.full((B * nkv * nsplit * 16 * dt,), float("nan"), device="cuda")
        pml = torch.full((B * nkv * nsplit * 16 * 2,), float("nan"), device="cuda")
        ops.attention(qf, nh * hd, None, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax,
                      B=B, Lq=1, Lkv=0, lkv_dev=i32([L]), Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, split_keys=SK,
                      nsplit=nsplit, part_o=po, part_ml=pml)
        for W, flag, wname in forms:
            for z in (1, 2):
                part = torch.full((z, B, nh * hd), float("nan"), device="cuda")
                fa = ops.fused_args(pro_mode=ops.PRO_ATTN_COMBINE, part_o=po, part_ml=pml, asplit=nsplit, head_dim=hd,
                                    dtw=dt, q_per_kv=nh // nkv, kv_heads=nkv)
                ops.gemm_fused(None, W, part, fa, epi=ops.EPI_F32 | flag, M=B, ksplit=z)
                _check(f"oproj_merge B={B} {wname} ksplit={z}", name, _heads(part.sum(0), B, 1, nh, hd), ref, unit, c)


# ------------------------------------------------------------------------------------ -inf and finfo.min masks
MASKED = [(2, 100, 4, 2, 64), (8, 130, 16, 1, 32)]       # the one-wave kernel; the LDS kernel (ONEWAVE / LDS above)
MASKS = ("causal", "left_pad", "window")


def _mask(kind, L, fill):
    """Additive [L][L]: causal; 40 keys of left padding (every row's first 32-key block wholly masked); a sliding
    window of 16 keys (late rows: many leading blocks wholly masked).  Every row keeps at least one key."""
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    if kind == "causal":
        hide = j > i
    elif kind == "left_pad":
        hide = (j < 40).expand(L, L)
    else:
        hide = (j > i) | (j < i - 15)
    assert bool((~hide).any(-1).all())
    return torch.zeros(L, L).masked_fill(hide, fill)


def _gauss(B, L, nh, nkv, hd, Smax, seed):
    g = torch.Generator().manual_seed(seed)
    q = R.bf16_exact(torch.randn(B, nh, L, hd, generator=g)).cuda()
    k = R.bf16_exact(torch.randn(B, nkv, Smax, hd, generator=g)).cuda()
    v = R.bf16_exact(torch.randn(B, nkv, Smax, hd, generator=g)).cuda()
    return q, k, v


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", MASKED, ids=_ids(MASKED))
def test_masks_of_minus_infinity(shape, kind):
    """An additive mask may hold -inf or finfo(float32).min (which the kernels' log2 e factor overflows to -inf): a
    row whose leading key blocks are wholly masked stays finite and within the bound of the fp64 reference under the
    same mask, and both fills give the same bits."""
    from pghip import ops
    B, L, nh, nkv, hd = shape
    Smax, kvd = _smax(L), nkv * hd
    q, k, v = _gauss(B, L, nh, nkv, hd, Smax, seed=21)
    qf, kc, vtc = _layout(q, k, v)
    outs = []
    for fill in (float("-inf"), torch.finfo(torch.float32).min):
        m = _mask(kind, L, fill).cuda()
        ref, budget = R.ref(q, k, v, hd ** -0.5, mask=m[None, None], lens=[L] * B)
        mask = m.expand(B, L, L).contiguous()
        o = torch.full((B * L, nh * hd), float("nan"), dtype=BF, device="cuda")
        ops.attention(qf, nh * hd, o, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax,
                      B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5, mask=mask, mask_bs=L * L, mask_rs=L)
        _check(f"mask {kind} fill={fill:.3g} {shape}", "gauss", _heads(o, B, L, nh, hd), ref, budget, R.C)
        outs.append(o)
    assert torch.equal(outs[0], outs[1])


# fp32 softmax of fp32 dot products against fp64: a logit's error is at most D 2^-24 sum_d |q_d k_d| scale (a sequential
# fp32 sum; about 64 * 6e-8 * 41 / 8 = 2e-5 at head_dim 64 with unit-variance inputs), it enters numerator and
# denominator, and exp of an argument up to about 12 adds 12 * 2^-23 + one ulp: under 1e-4 relative in all
PROBS_RTOL = 1e-4


@pytest.mark.parametrize("kind", ["left_pad", "window"])
@pytest.mark.parametrize("shape", MASKED, ids=_ids(MASKED))
def test_attn_probs_masks_of_minus_infinity(shape, kind):
    """pg_attn_probs (probs = 1) under the same masks: finite, masked keys exactly 0, the rest within PROBS_RTOL of the
    fp64 softmax, both fills alike."""
    from pghip import ops
    B, L, nh, nkv, hd = shape
    Smax, kvd = _smax(L), nkv * hd
    q, k, v = _gauss(B, L, nh, nkv, hd, Smax, seed=22)
    qf, kc, _ = _layout(q, k, v)
    g = nh // nkv
    for fill in (float("-inf"), torch.finfo(torch.float32).min):
        m = _mask(kind, L, fill).cuda()
        p = ops.attn_probs(qf, nh * hd, kc, Smax * kvd, hd, kvd, B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd,
                           scale=hd ** -0.5, mask=m.expand(B, L, L).contiguous(), mask_bs=L * L, mask_rs=L, probs=True)
        s = (q.double() @ k[:, :, :L].double().repeat_interleave(g, 1).transpose(-1, -2)) * hd ** -0.5 + m.double()
        ref = torch.softmax(s, -1)
        assert torch.isfinite(p).all(), (kind, fill)
        hidden = (m != 0).expand_as(p)
        assert bool((p[hidden] == 0).all())
        rel = float(((p.double() - ref).abs() / ref.clamp_min(1e-300))[~hidden].max())
        print(f"probs {kind} fill={fill:.3g} {shape}: worst relative error {rel:.3g}")
        assert rel <= PROBS_RTOL, (kind, fill, rel)
