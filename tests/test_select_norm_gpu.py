"""The end of every decode step on the HIP device: the final norm (pg_norm_residual / _fp8, all four kernel
instantiations, row_map, write_resid, slab rounds, column edges), the greedy selectors (pg_argmax, pg_argmax_embed,
pg_argmax_pairs + pg_argmax_merge) and the top-p sampler (pg_topp_sample), each against the float64 / torch.argmax
references of tests/select_ref.py at the shapes where the kernels take another path."""
import numpy as np
import pytest
import torch

import select_ref as R

pytestmark = pytest.mark.gpu

F32_BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def _rng_row(V, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(V) * scale).astype(np.float32)


# ====================================================================== top-p sampler
def _topp(logits, u, T, P, probs=False, **st):
    """One pg_topp_sample launch: (ids [B], probs_out [B][V] or None) on the host."""
    from pghip import ops
    B, V = logits.shape
    ids = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    pr = torch.full((B, V), float("nan"), device="cuda") if probs else None
    ops.topp_sample(logits, ids, u, temperature=T, top_p=P, probs_out=pr, **st)
    return ids.cpu().numpy(), (pr.cpu().numpy() if probs else None)


def _check_rows(x, u, T, P, exact_kept=False):
    """x [B][V] fp32 (host), u [B]: one launch, every row against the float64 contract.  Returns the kept masks."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = np.asarray(u, dtype=np.float32)
    ids, pr = _topp(torch.from_numpy(x).cuda(), torch.from_numpy(u)[None].cuda(), T, P, probs=True)
    kepts = []
    for b in range(x.shape[0]):
        ref = R.TopPRow(x[b], T, P)
        kept = pr[b] != 0
        assert ref.check_kept(kept) == [], (b, ref.check_kept(kept))
        if exact_kept:
            assert np.array_equal(kept, ref.K), (b, np.nonzero(kept != ref.K)[0][:8])
        assert not ref.check_draw(u[b], ids[b], kept).any(), (b, float(u[b]), int(ids[b]))
        kepts.append(kept)
    return ids, np.stack(kepts)


@pytest.mark.parametrize("P", [1.0, 0.9])
def test_topp_boundary_sweep(P):
    """Every fp32 uniform within +-256 ulp of each thread-chunk boundary of the CDF (V = 8197: 9 tokens per thread)
    plus 4096 evenly spaced ones, one launch over a stride-0 expanded row: every draw inside the contract.
    With per-thread intervals [scan[t] - mine, scan[t]) 299 of the 470926 draws (top_p = 1) and 268 of the 469644
    (top_p = 0.9) fell into a gap between two intervals and returned the last kept token of the vocabulary; with
    [scan[t-1], scan[t]) 0 and 220 still did (an empty chunk's scan entry can exceed its neighbour's)."""
    V, T = 8197, 1.0
    x = _rng_row(V, 1)
    assert (x.max() - x.min()) / T <= 32
    ref = R.TopPRow(x, T, P)
    row = torch.from_numpy(x).cuda()[None]
    _, pr = _topp(row, torch.tensor([[0.5]], device="cuda"), T, P, probs=True)
    kept = pr[0] != 0
    assert ref.check_kept(kept) == [], ref.check_kept(kept)
    u = np.concatenate([R.ulp_window(ref.chunk_starts(kept), 256),
                        (np.arange(4096, dtype=np.float64) / 4096).astype(np.float32)])
    B = u.shape[0]
    assert 450_000 < B < 550_000
    ids, _ = _topp(row.expand(B, V), torch.from_numpy(u)[None].cuda(), T, P)
    bad = ref.check_draw(u, ids, kept)
    last = int(np.nonzero(kept)[0].max())
    print(f"topp sweep top_p={P}: {int(bad.sum())} of {B} draws violate the contract "
          f"({int((bad & (ids == last)).sum())} of them drew the last kept token {last})")
    assert not bad.any(), (int(bad.sum()), u[bad][:5].tolist(), ids[bad][:5].tolist())


def test_topp_batch_stride_and_state_advance():
    """B = 5 distinct rows at ld = 1024 != V = 1000 (+1e9 past V), uniforms and hist [3][B], five calls from step 0:
    each row's draw against uniforms[min(step, 2)], hist written only while step < 3 (guard rows untouched),
    pos / kv_len / step advance, probs_out row b at b * V."""
    B, V, T, P = 5, 1000, 0.7, 0.9
    wide = np.full((B, 1024), 1e9, dtype=np.float32)
    wide[:, :V] = np.stack([_rng_row(V, 10 + b, 2.0) for b in range(B)])
    x = wide[:, :V]
    assert ((x.max(1) - x.min(1)) / T).max() <= 32
    logits = torch.from_numpy(wide).cuda()[:, :V]
    assert logits.stride(0) == 1024
    u = np.random.default_rng(3).random((3, B), dtype=np.float32)
    ud = torch.from_numpy(u).cuda()
    guard = torch.full((5, B), -7, dtype=torch.int64, device="cuda")
    hist = guard[1:4]
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    pos = torch.arange(10, 10 + B, dtype=torch.int32, device="cuda")
    kv = torch.tensor([20], dtype=torch.int32, device="cuda")
    refs = [R.TopPRow(np.ascontiguousarray(x[b]), T, P) for b in range(B)]
    seen = []
    for k in range(5):
        ids, pr = _topp(logits, ud, T, P, probs=True, hist=hist, step=step, pos=pos, kv_len=kv)
        for b, ref in enumerate(refs):
            kept = pr[b] != 0
            assert ref.check_kept(kept) == [], (k, b, ref.check_kept(kept))
            assert not ref.check_draw(u[min(k, 2), b], ids[b], kept).any(), (k, b, int(ids[b]))
            # the renormalised distribution itself: exp as exp2 (2^-19), the kept sum (per + 10 adds), one division
            q = np.where(kept, ref.p, 0.0)
            q /= q.sum()
            assert np.all(np.abs(pr[b] - q) <= 2 * ref.tol * q), (k, b)
        seen.append(ids)
        h = guard.cpu().numpy()
        assert (h[0] == -7).all() and (h[4] == -7).all()
        for r in range(3):
            assert (h[1 + r] == (seen[r] if r <= k else -7)).all(), (k, r)
        assert step.item() == k + 1 and kv.item() == 21 + k
        assert pos.cpu().tolist() == [10 + b + k + 1 for b in range(B)]
    # steps 2, 3 and 4 read the same uniforms row, so they draw the same tokens
    assert (seen[2] == seen[3]).all() and (seen[3] == seen[4]).all()


@pytest.mark.parametrize("V", [1, 5, 1023, 1025])
def test_topp_small_and_odd_vocabularies(V):
    x = np.stack([_rng_row(V, 20 + b) for b in range(4)])
    if V >= 5:
        x[1, [0, V - 1]] = -np.inf                        # -inf logits are never kept (check_kept: p == 0)
        x[2, 1:4] = x[2].max() + 1.0                      # a tied maximum
    u = np.array([0.0, F32_BELOW_1, 0.37, 0.8125], dtype=np.float32)
    _check_rows(x, u, 1.0, 0.9)
    _check_rows(x, u[::-1].copy(), 1.0, 0.5)


def test_topp_top_p_zero_and_one():
    V = 1025
    # a narrow row: every token carries ~1e-3 of the mass, far above the rounding of the kernel's mass sums, so the
    # kept sets are exact
    x = np.stack([_rng_row(V, 30 + b, 0.5) for b in range(4)])
    x[:, [7, 600, 1024]] = -np.inf
    x[:, [3, 512, 1023]] = 4.0                            # the maximal tie group, across the threads' chunks
    u = np.array([0.0, F32_BELOW_1, 0.34, 0.67], dtype=np.float32)
    ids, kept = _check_rows(x, u, 1.0, 0.0, exact_kept=True)
    assert np.nonzero(kept[0])[0].tolist() == [3, 512, 1023]
    assert ids.tolist() == [3, 1023, 512, 1023]           # thirds of the CDF
    ids, kept = _check_rows(x, u, 1.0, 1.0, exact_kept=True)
    assert (kept == np.isfinite(x)).all()


def test_topp_low_temperature_underflow():
    """T = 0.01 with logit gaps of 2: every exp but the maximum's underflows to zero, any uniform draws the argmax."""
    V = 1025
    x = np.stack([np.random.default_rng(40 + b).permutation(V).astype(np.float32) * 2 for b in range(4)])
    u = np.array([0.0, F32_BELOW_1, 0.5, 0.999], dtype=np.float32)
    ids, kept = _check_rows(x, u, 0.01, 0.9, exact_kept=True)
    assert ids.tolist() == x.argmax(1).tolist() and (kept.sum(1) == 1).all()


def test_topp_tie_group_straddling_the_cut_is_kept_whole():
    V, T = 1025, 1.0
    x = torch.from_numpy(_rng_row(V, 50, 2.0)).to(torch.bfloat16).float().numpy()
    x[x == 2.0] = 1.9921875                               # the bf16 value below 2: the group below is exactly 7 wide
    tie = [3, 200, 511, 512, 700, 1023, 1024]
    x[tie] = 2.0
    probe = R.TopPRow(x, T, 0.5)
    P = float(probe.before[3] + 3.5 * probe.p[3])         # the sorted cumulative mass crosses top_p inside the group
    assert 0.1 < P < 0.95 and probe.p[3] > 1e-4
    u = np.array([0.0, F32_BELOW_1, 0.25, 0.75], dtype=np.float32)
    _, kept = _check_rows(np.stack([x] * 4), u, T, P, exact_kept=True)
    assert kept[0][tie].all() and not kept[0][x < 2.0].any()


@pytest.mark.parametrize("T", [0.0, -1.0])
def test_topp_rejects_non_positive_temperature(T):
    with pytest.raises(RuntimeError):
        _topp(torch.zeros(1, 8, device="cuda"), torch.full((1, 1), 0.5, device="cuda"), T, 0.9)


# ====================================================================== argmax family
def _am_state(B, hist_rows=3, step0=1):
    guard = torch.full((hist_rows + 2, B), -7, dtype=torch.int64, device="cuda")
    return dict(hist=guard[1:1 + hist_rows], step=torch.tensor([step0], dtype=torch.int32, device="cuda"),
                pos=torch.arange(B, dtype=torch.int32, device="cuda"),
                kv_len=torch.tensor([9], dtype=torch.int32, device="cuda")), guard


def _state_host(st, guard):
    return [t.cpu() for t in (guard, st["step"], st["pos"], st["kv_len"])]


def _am_rows(V, B, seed):
    """Rows where an argmax kernel goes wrong: all-equal, all -inf, the maximum last, the maximum duplicated across
    the first pass's chunk edge (per = ((V + 63) / 64 + 3) & ~3 columns per chunk), then seeded normals."""
    x = torch.randn(max(B, 5), V, generator=torch.Generator().manual_seed(seed))
    x[0] = 1.5
    x[1] = float("-inf")
    x[2, V - 1] = 50.0
    per = ((V + 63) // 64 + 3) & ~3
    if per < V:
        x[3, per - 1] = 40.0
        x[3, per] = 40.0
    if 2 * per < V:
        x[4, 2 * per] = 40.0
        x[4, per - 1] = 40.0
    return x


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("V,pad", [(1, 3), (3, 1), (255, 1), (257, 3), (1000, 0), (1000, 64)])
def test_argmax_and_argmax_embed_small_and_odd_shapes(V, pad, B):
    """ld = V rounded up to 4 (and V + 64), +1e9 in the padding columns; pg_argmax against torch.argmax, the state
    advance, and pg_argmax_embed bit-equal to pg_argmax + pg_embed_merge (H = 8)."""
    from pghip import ops
    ld, H = V + pad, 8
    assert ld % 4 == 0
    rows = _am_rows(V, 17, V)
    g = torch.Generator().manual_seed(V)
    embed = (torch.randn(V, H, generator=g) * 0.05).to(torch.bfloat16).cuda()
    feat = torch.randn(1, H, generator=g).cuda()
    kw = dict(image_id=V - 1, pad_id=0, img_scale=H ** -0.5, normalizer=H ** 0.5)
    for r0 in ([0] if B == 17 else range(5)):             # B = 1: each of the special rows on its own
        buf = torch.full((B, ld), 1e9)
        buf[:, :V] = rows[r0:r0 + B]
        x = buf.cuda()[:, :V]
        want = torch.argmax(rows[r0:r0 + B], -1)
        if r0 == 0:
            assert want[0].item() == 0 and (B == 1 or (want[1].item() == 0 and want[2].item() == V - 1))
        outs = []
        for fused in (True, False):
            ids = torch.full((B,), -5, dtype=torch.int64, device="cuda")
            ws = torch.empty(B * 64 * 2, device="cuda")
            res = torch.full((B, H), float("nan"), device="cuda")
            st, guard = _am_state(B)
            if fused:
                ops.argmax_embed(x, ids, ws, embed, feat, 1, res, **kw, **st)
            else:
                ops.argmax(x, ids, ws, **st)
                ops.embed_merge(ids, None, embed, feat, 1, res, **kw)
            assert ids.cpu().tolist() == want.tolist(), (r0, fused)
            h = guard.cpu()
            assert h[2].tolist() == want.tolist() and (h[[0, 1, 3, 4]] == -7).all()
            assert st["step"].item() == 2 and st["kv_len"].item() == 10
            assert st["pos"].cpu().tolist() == list(range(1, B + 1))
            outs.append(res.cpu())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def _shards(x, world):
    """x [B][V] (host) -> `world` device tensors [B][V / world], each in its own 4-column-aligned buffer whose
    padding columns hold +1e9, and their vocabulary offsets."""
    B, V = x.shape
    n = V // world
    assert n * world == V
    out = []
    for r in range(world):
        buf = torch.full((B, (n + 3) & ~3), 1e9)
        buf[:, :n] = x[:, r * n:(r + 1) * n]
        out.append((buf.cuda()[:, :n], r * n))
    return out


def _pairs_merge(x, world, st, base=0):
    from pghip import ops
    B = x.shape[0]
    pairs = torch.full((world, B, 2), float("nan"), device="cuda")
    ws = torch.empty(B * 64 * 2, device="cuda")
    for r, (sh, off) in enumerate(_shards(x, world)):
        ops.argmax_pairs(sh, ws, pairs[r], vocab_offset=base + off)
    ids = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    ops.argmax_merge(pairs, ids, world=world, **st)
    return ids.cpu(), pairs.cpu()


@pytest.mark.parametrize("world", [1, 2, 8])
def test_argmax_pairs_and_merge_on_one_device(world):
    from pghip import ops
    V, B = 1000, 6
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(70))
    x[0, 100] = 60.0
    x[0, 900] = 60.0                                      # a global tie across shards: the lower index wins
    x[1, V - 1] = 60.0
    x[2, :125] = float("-inf")                            # one shard (of 8) all -inf
    x[3] = float("-inf")
    x[4] = -2.0
    want = torch.argmax(x, -1)
    assert want[0].item() == 100 and want[3].item() == 0 and want[4].item() == 0 and want[2].item() >= 125
    xd = x.cuda()
    ws = torch.empty(B * 64 * 2, device="cuda")
    # the state advance equals pg_argmax's, at a recorded step and at one past the history (hist_rows = 2)
    for step0 in (1, 2):
        st_m, guard_m = _am_state(B, hist_rows=2, step0=step0)
        st_a, guard_a = _am_state(B, hist_rows=2, step0=step0)
        ids, pairs = _pairs_merge(x, world, st_m)
        ida = torch.full((B,), -5, dtype=torch.int64, device="cuda")
        ops.argmax(xd, ida, ws, **st_a)
        assert ids.tolist() == want.tolist() and ida.cpu().tolist() == want.tolist()
        for a, b in zip(_state_host(st_m, guard_m), _state_host(st_a, guard_a)):
            assert torch.equal(a, b)
        h = guard_m.cpu()
        assert (h[[0, 1, 3]] == -7).all()
        assert h[2].tolist() == (want.tolist() if step0 == 1 else [-7] * B)
        assert st_m["step"].item() == step0 + 1
        n = V // world
        for r in range(world):                            # each shard's pair: its own maximum and its global index
            sh = x[:, r * n:(r + 1) * n]
            assert torch.equal(pairs[r, :, 0], sh.max(-1).values)
            assert pairs[r, :, 1].tolist() == (torch.argmax(sh, -1) + r * n).tolist()


def test_argmax_pairs_indices_just_below_the_float_exact_limit():
    from pghip import ops
    V, B = 1000, 3
    base = (1 << 24) - 1001
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(71))
    x[1, V - 1] = 60.0
    x[2, V - 2] = 60.0
    want = torch.argmax(x, -1) + base
    ids, pairs = _pairs_merge(x, 1, {}, base=base)
    assert ids.tolist() == want.tolist() and ids[1].item() == (1 << 24) - 2
    assert pairs[0, :, 1].tolist() == want.tolist()
    with pytest.raises(RuntimeError):                     # vocab_offset + V >= 2^24: the float index is not exact
        ops.argmax_pairs(x.cuda(), torch.empty(B * 64 * 2, device="cuda"), torch.empty(B, 2, device="cuda"),
                         vocab_offset=(1 << 24) - 1000)


@pytest.mark.parametrize("V", [3, 1000])
def test_argmax_rows_with_no_comparable_value(V):
    """An all-NaN row returns id 0 from every selector (no id outside [0, V) reaches out_ids, hist or pairs); a NaN
    among comparable values is skipped."""
    from pghip import ops
    B, H = 18, 8
    nan = float("nan")
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(72))
    x[0] = nan
    x[1, 0] = nan                                         # skipped: the winner is among the rest
    x[2, V - 1] = nan
    x[3] = float("-inf")
    x[3, 0] = nan                                         # NaN, then -inf only: the first -inf
    x[17] = nan                                           # a row of the final pass's second round of waves
    want = torch.argmax(torch.where(torch.isnan(x), torch.tensor(float("-inf")), x), -1)
    want[0] = want[17] = 0
    want[3] = 1
    buf = torch.full((B, (V + 3) & ~3), 1e9)
    buf[:, :V] = x
    xd = buf.cuda()[:, :V]
    g = torch.Generator().manual_seed(V)
    embed = (torch.randn(V, H, generator=g) * 0.05).to(torch.bfloat16).cuda()
    kw = dict(image_id=-1, pad_id=-2, img_scale=1.0, normalizer=H ** 0.5)
    ws = torch.empty(B * 64 * 2, device="cuda")
    outs = []
    for fused in (True, False):
        ids = torch.full((B,), -5, dtype=torch.int64, device="cuda")
        res = torch.full((B, H), nan, device="cuda")
        st, guard = _am_state(B)
        if fused:
            ops.argmax_embed(xd, ids, ws, embed, None, 0, res, **kw, **st)
        else:
            ops.argmax(xd, ids, ws, **st)
            ops.embed_merge(ids, None, embed, None, 0, res, **kw)
        assert ids.cpu().tolist() == want.tolist(), fused
        assert guard[2].cpu().tolist() == want.tolist()
        outs.append(res.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], embed.cpu().float()[want] * H ** 0.5)
    for world in ((1, 3) if V == 3 else (1, 2, 8)):
        st, guard = _am_state(B)
        ids, pairs = _pairs_merge(x, world, st)
        assert ids.tolist() == want.tolist(), world
        assert guard[2].cpu().tolist() == want.tolist()
        n = V // world
        for r in range(world):
            idx = pairs[r, :, 1]
            assert ((idx >= r * n) & (idx < (r + 1) * n)).all(), (world, r)
            # a shard's value is NaN exactly where the shard has no comparable value: it loses the merge to every other
            assert torch.equal(torch.isnan(pairs[r, :, 0]), torch.isnan(x[:, r * n:(r + 1) * n]).all(-1)), (world, r)
        assert pairs[0, 0, 1].item() == 0.0


# ====================================================================== residual norms
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _norm_case(mode, M_out, H, nsplit, *, M_in=None, row_map=None, write_resid=True, seed=0):
    """pg_norm_residual and pg_norm_residual_fp8 on the same inputs, against the float64 norm of the fp32 slab sum:
    out_f32 per row, bf16 out == RNE(out_f32), the padding columns of out (ldo > H), the residual bit for bit
    (written rows and all the others), fp8 bytes + scales == pg_quant_fp8 of the bf16 output."""
    from pghip import ops
    M_in = M_out if M_in is None else M_in
    g = torch.Generator().manual_seed(1000 * mode + H + nsplit + seed)
    # rows of different scales and a non-zero mean, so one bad row cannot hide under another's magnitude
    rs = 10.0 ** (torch.rand(M_in, 1, generator=g) * 4 - 2)
    resid = (torch.randn(M_in, H, generator=g) + 0.5) * rs
    part = torch.randn(max(nsplit, 1), M_in, H, generator=g) * 0.3 * rs
    w = torch.randn(H, generator=g) * 0.1 + (1 if mode == 0 else 0)
    b = torch.randn(H, generator=g) * 0.1 if mode == 0 else None
    rows = list(range(M_out)) if row_map is None else list(row_map)
    assert len(rows) == M_out
    rm = None if row_map is None else torch.tensor(rows, dtype=torch.int32, device="cuda")
    x32 = R.slab_sum_f32(resid.numpy()[rows], part.numpy()[:, rows], nsplit)
    ref = R.norm_f64(x32, w.numpy(), None if b is None else b.numpy(), mode, 1e-6)
    resid_want = resid.clone()
    if write_resid and nsplit > 0:
        resid_want[rows] = torch.from_numpy(x32)
    wd, bd, pd = w.cuda(), (None if b is None else b.cuda()), part.cuda()
    kw = dict(b=bd, mode=mode, partials=pd if nsplit else None, nsplit=nsplit, row_map=rm, write_resid=write_resid)

    r1 = resid.cuda()
    Hp = (H + 15) & ~7                                    # ldo > H, a multiple of 8 (pg_quant_fp8 reads it below)
    obuf = torch.full((M_out, Hp), 0.0, dtype=torch.bfloat16, device="cuda")
    obuf[:, H:] = -3.0
    of = torch.full((M_out, H), float("nan"), device="cuda")
    ops.norm_residual(r1, wd, out=obuf[:, :H], out_f32=of, **kw)
    e = R.row_err(of.cpu().numpy(), ref)
    assert e.max() <= 1e-5, (int(e.argmax()), float(e.max()))
    assert torch.equal(_bits(obuf[:, :H]), _bits(of.to(torch.bfloat16)))
    assert (obuf[:, H:] == -3.0).all()
    assert torch.equal(_bits(r1.cpu()), _bits(resid_want))

    r2 = resid.cuda()
    q = torch.full((M_out, H + 4), 0xA5, dtype=torch.uint8, device="cuda")
    s = torch.full((M_out,), float("nan"), device="cuda")
    ops.norm_residual_fp8(r2, wd, q, s, **kw)
    obuf[:, H:] = 0.0                                     # zero columns change neither the row's amax nor its bytes
    q_ref, s_ref = ops.quant_fp8(obuf)
    assert torch.equal(_bits(s), _bits(s_ref))
    assert torch.equal(q[:, :H], q_ref[:, :H]) and (q[:, H:] == 0xA5).all()
    assert torch.equal(_bits(r2.cpu()), _bits(resid_want))


# (M_out, H, nsplit) -> norm_residual_kernel<slabs per round, float4 slots>: deep (8 slabs) needs nsplit > 2 and
# M_out <= 2048, wide (4 slots) H > 2048
INSTANTIATIONS = [(3, 2048, 16),      # <8, 2>, two full rounds
                  (3, 4096, 17),      # <8, 4>, a ragged third round
                  (2049, 128, 3),     # <2, 2>, two rounds
                  (2049, 2052, 3)]    # <2, 4>, two rounds, 513 float4 columns
SLAB_COUNTS = [(5, 1152, n) for n in (0, 1, 2, 8, 9)]                   # <2, 2> up to 2 slabs, <8, 2> above
COLUMN_EDGES = [(3, H, 1) for H in (4, 1028, 2052, 3072, 4096)]         # <2, 2> to 2048 columns, <2, 4> above


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,H,nsplit", INSTANTIATIONS + SLAB_COUNTS + COLUMN_EDGES)
def test_norm_residual_instantiations_slab_rounds_and_column_edges(M, H, nsplit, mode):
    _norm_case(mode, M, H, nsplit)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H", [1028, 4096])
@pytest.mark.parametrize("row_map,write_resid", [([39, 0, 17, 17], False), ([39, 0, 17, 5], True)])
def test_norm_residual_row_map_gathers_rows(row_map, write_resid, H, mode):
    """M_part = 40 input rows, M_out = 4: out is indexed by the output row, resid and partials by the mapped row;
    rows the map does not name (all rows when write_resid = 0) stay bit-identical."""
    _norm_case(mode, 4, H, 3, M_in=40, row_map=row_map, write_resid=write_resid)


@pytest.mark.parametrize("mode", [0, 1])
def test_norm_residual_write_resid_off_leaves_the_residual(mode):
    _norm_case(mode, 5, 1152, 3, write_resid=False)
    _norm_case(mode, 3, 4096, 9, write_resid=False)


@pytest.mark.parametrize("fp8", [False, True])
def test_norm_residual_rejections(fp8):
    from pghip import ops

    def run(H, mode=1, bias=False, nsplit=0, partials=False):
        resid = torch.zeros(2, H, device="cuda")
        w = torch.zeros(H, device="cuda")
        kw = dict(b=w if bias else None, mode=mode, nsplit=nsplit,
                  partials=torch.zeros(max(nsplit, 1), 2, H, device="cuda") if partials else None)
        if fp8:
            ops.norm_residual_fp8(resid, w, torch.empty(2, (H + 3) & ~3, dtype=torch.uint8, device="cuda"),
                                  torch.empty(2, device="cuda"), **kw)
        else:
            ops.norm_residual(resid, w, out=torch.empty(2, H, dtype=torch.bfloat16, device="cuda"), **kw)

    run(8)                                                # the accepted neighbours of the refused calls
    run(4096)
    run(8, mode=0, bias=True)
    run(8, nsplit=1, partials=True)
    for bad in (dict(H=4100), dict(H=6), dict(H=8, mode=0), dict(H=8, nsplit=1)):
        with pytest.raises(RuntimeError):
            run(**bad)
    torch.cuda.synchronize()
