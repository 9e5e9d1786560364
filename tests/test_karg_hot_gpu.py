"""The hot argument header of the batch-1 decode kernels (csrc/common.h PG_KARG_HOT).  The gate/up, down and lm_head
GEMVs on the exponent-coded packs and the argmax + embed finaliser take what their first loads need as leading scalar
parameters, filled by the launchers from the structs they always built; every other GEMV launch (q|k|v and o_proj
among them: they lost with a header, DESIGN A) passes the same struct first instead of last, and the argmax partial
kernel takes its arguments as one struct.  No arithmetic changed, so every comparison is torch.equal, and the
reference is a form none of this reaches or reaches differently:

  * GEMV forms: the same launch at M = 5 rows with the bf16 fragment pack -- two tiles per workgroup, the struct
    signature -- whose first rows must equal the M = 1 and M = 2 launches of the fragment pack, the 13-bit pack and a
    mixed narrow / wide 12-bit pack.  (Sums of squares handed to pro_mode 4 are small integers: the row forms add them
    in different orders, and integer-valued floats add exactly in any.)
  * argmax + embed: pg_argmax followed by pg_embed_merge.
  * end to end: the captured batch-1 decode graph against tokens and logits recorded from the commit before.

The cases walk the header's fields -- each one null, set, and switching meaning where it can -- and the struct's
neighbours of those fields (the cache slot word, amax_zero, status) at the smallest shapes that still take the batch-1
path: K = 512 is one 128-k block per wave (the generic block loop), K = 2048 the straight-line forms of 8 chunks per
wave (4 at split 2) that the full-size model runs."""
import copy
import os

import pytest
import torch

from test_frag12_gpu import weights_of

pytestmark = pytest.mark.gpu

MR = 5            # rows of the reference launch


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def fx_rows(M, N, seed):
    """a fixed-point accumulator [M][N] holding values of order 1"""
    return (rnd(M, N, seed=seed, dtype=torch.float32).double() * 2.0 ** 32).round().to(torch.int64)


def matrices(N, K, packs=True):
    """(name, W, layout flag, N / K keywords) of one matrix: fragment pack, 13-bit pack, mixed narrow / wide 12-bit pack"""
    from pghip import ops
    from pghip.weights import frag13_pack
    w, wf, w12 = weights_of("mixed", N, K)
    out = [("frag", wf, ops.W_FRAG, {})]
    if packs:
        w13 = frag13_pack(w)
        assert w13 is not None
        out += [("w13", w13, ops.W_FRAG13, dict(N=N, K=K)), ("w12", w12, ops.W_FRAG13 | ops.W_FRAG12, dict(N=N, K=K))]
    return out


def check(launch, N, K, packs=True, rows=(1, 2)):
    """launch(W, flag, nk, M) -> tensors with M leading rows.  The reference runs once, at MR rows of the fragment
    pack; every matrix at every row count must reproduce its first rows bit for bit."""
    mats = matrices(N, K, packs)
    want = launch(mats[0][1], mats[0][2], mats[0][3], MR)
    torch.cuda.synchronize()
    assert any(bool(t.float().abs().sum() > 0) for t in want)
    for name, W, flag, nk in mats:
        for M in rows:
            got = launch(W, flag, nk, M)
            torch.cuda.synchronize()
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(want, got)):
                assert torch.equal(a[:M], b[:M]), (name, M, i, N, K)


def check_ss(ss, res):
    """PG_EPI_F32_FIN's sums of squares [M][entries] of the finalised residual res [M][N].  Not part of the bit-exact
    comparison: the reference form writes one entry per tile pair, the batch-1 form one per tile, and each adds its 16
    or 32 squares in its own order -- so they are held against the fp64 sum over the entry's columns, to the error of
    adding 32 non-negative fp32 terms (32 * 2^-24, doubled)."""
    M, n = ss.shape
    want = res[:M].double().pow(2).reshape(M, n, -1).sum(-1)
    assert bool(((ss.double() - want).abs() <= want * 2.0 ** -18).all())


# ---------------------------------------------------------------------------------------------------------- q|k|v
HD, NH, NKV, SMAX = 16, 1, 1, 32
NQKV = (NH + 2 * NKV) * HD                               # 48: three tiles


def qkv_launch(K, *, pro4=False, fx=False, resid=True, slot="shared", zero=False):
    from pghip import engine, ops
    cos_t, sin_t = engine.rope_tables(HD, 64, 10000.0, "cuda")
    resid_t = rnd(MR, K, seed=1, dtype=torch.float32)
    fx_t = fx_rows(MR, K, 7)
    nw = rnd(K, scale=0.1, seed=2, dtype=torch.float32)
    x = rnd(MR, K, seed=8)
    ss = torch.arange(1, MR * 8 + 1, dtype=torch.float32, device="cuda").reshape(MR, 8) * 64.0
    pos = torch.tensor([5, 9, 2, 30, 17], dtype=torch.int32, device="cuda")
    slot_t = {"null": None, "shared": torch.tensor([3], dtype=torch.int32, device="cuda"),
              "rows": torch.tensor([3, 0, 7, 1, 30], dtype=torch.int32, device="cuda")}[slot]

    def launch(W, flag, nk, M):
        kc, vtc = rnd(MR, SMAX, NKV * HD, seed=3), rnd(MR, NKV * HD, SMAX, seed=4)
        kd, vd = rnd(MR, SMAX * NKV * HD, seed=5), rnd(MR, SMAX * NKV * HD, seed=6)
        q = torch.zeros(MR, NH * HD, dtype=torch.bfloat16, device="cuda")
        dirty = torch.full((64,), 0x55, dtype=torch.int32, device="cuda")
        kw = dict(eps=1e-6, head_dim=HD, cos_t=cos_t, sin_t=sin_t, pos=pos, rows_per_batch=1, kc=kc, vtc=vtc, kd=kd,
                  vd=vd, smax=SMAX, q_heads=NH, kv_heads=NKV, slot_base=2 if slot == "null" else 0)
        if slot_t is not None:
            kw.update(slot_dev=slot_t)
        if zero:
            kw.update(amax_zero=dirty, amax_zero_n=dirty.numel())
        if pro4:
            kw.update(pro_mode=ops.PRO_X_RSTD, ss_in=ss, ss_ld=8, ss_n=8)
        else:
            kw.update(pro_mode=ops.PRO_RMSNORM, nsplit=0, norm_w=nw)
            if resid:
                kw.update(resid_in=resid_t)
            if fx:
                kw.update(fx=fx_t)
        epi = ops.EPI_QKV_ROPE | flag | (ops.SLOT_ROWS if slot == "rows" else 0)
        ops.gemm_fused(x if pro4 else None, W, q, ops.fused_args(**kw), epi=epi, M=M, **nk)
        if zero:
            assert not bool(dirty.any())
        return q, kc, vtc, kd, vd
    return launch


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("case", [dict(), dict(fx=True), dict(fx=True, resid=False), dict(slot="null"),
                                  dict(slot="rows"), dict(zero=True)],
                         ids=["resid", "resid+fx", "fx", "slot-null", "slot-rows", "amax-zero"])
def test_qkv_rmsnorm_prologue(K, case):
    """PG_EPI_QKV_ROPE, pro_mode 1 (struct-first signature on every pack): fx / resid_in null and set; the cache slot
    word null, shared and per row; amax_zero set (the step's first launch, which runs without fx)."""
    check(qkv_launch(K, **case), NQKV, K)


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("slot", ["shared", "rows"])
def test_qkv_rstd_prologue(K, slot):
    """PG_EPI_QKV_ROPE, pro_mode 4 (x' and sums of squares from a finalising down projection)."""
    check(qkv_launch(K, pro4=True, slot=slot), NQKV, K, packs=False)


# ---------------------------------------------------------------------------------------------------------- o_proj
@pytest.mark.parametrize("N", [32, 48])
@pytest.mark.parametrize("form", ["fx_add-1", "fx_add-2", "f32_add-1", "f32_fin-1", "f32_fin-2"])
def test_o_proj_attention_merge_prologue(form, N):
    """pro_mode 2 (struct-first signature) under the three epilogues the decode step has used, K split 1 and 2 (the
    float-atomic F32_ADD only unsplit: its split order is not fixed)."""
    from pghip import ops
    epi_name, ks = form.split("-")
    ks = int(ks)
    nh, nkv, hd, S, dt = 8, 1, 256, 4, 256
    K, tiles = nh * hd, N // 16
    po = rnd(MR * nkv * S * 16 * dt, seed=31, dtype=torch.float32)
    ml = torch.stack([rnd(MR * nkv * S * 16, seed=32, dtype=torch.float32),
                      rnd(MR * nkv * S * 16, seed=33, dtype=torch.float32).abs() + 0.5], -1).contiguous()
    bias = rnd(N, seed=34, dtype=torch.float32)

    def launch(W, flag, nk, M):
        kw = dict(pro_mode=ops.PRO_ATTN_COMBINE, part_o=po, part_ml=ml, asplit=S, head_dim=hd, dtw=dt,
                  q_per_kv=nh // nkv, kv_heads=nkv)
        if epi_name == "fx_add":
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            acc = fx_rows(MR, N, 35)
            ops.gemm_fused(None, W, acc, ops.fused_args(status=st, **kw), epi=ops.EPI_FX_ADD | flag, M=M, ksplit=ks,
                           bias=bias, **nk)
            assert int(st) == 0
            return (acc,)
        if epi_name == "f32_add":
            acc = rnd(MR, N, seed=36, dtype=torch.float32)
            ops.gemm_fused(None, W, acc, ops.fused_args(**kw), epi=ops.EPI_F32_ADD | flag, M=M, ksplit=ks, **nk)
            return (acc,)
        part = torch.zeros(ks, M, N, device="cuda")
        cnt = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        res = rnd(MR, N, seed=37, dtype=torch.float32)[:M].contiguous()
        ss = torch.zeros(M, tiles, device="cuda")
        ops.gemm_fused(None, W, part, ops.fused_args(fin_cnt=cnt, fin_resid=res, ss_out=ss, ss_ld=tiles, **kw),
                       epi=ops.EPI_F32_FIN | flag, M=M, ksplit=ks, **nk)
        assert not bool(cnt.any())
        if M <= 4:
            check_ss(ss, res)
        return (res,)

    # (the packs implement FX_ADD only for this prologue)
    check(launch, N, K, packs=epi_name == "fx_add")


# ---------------------------------------------------------------------------------------------------------- gate / up
@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("case", ["resid", "resid+fx", "fx"])
def test_gate_up_rmsnorm_prologue(case, N, K):
    """PG_EPI_BF16_GELU_MUL, pro_mode 1, the interleaved tile pair per workgroup: fx null / set, resid_in null with fx.
    (The fragment pack's own gate/up launch keeps the struct-only signature at every row count; the packs' is hot.)"""
    from pghip import ops
    resid = rnd(MR, K, seed=11, dtype=torch.float32)
    fx = fx_rows(MR, K, 13)
    nw = rnd(K, scale=0.1, seed=12, dtype=torch.float32)

    def launch(W, flag, nk, M):
        h = torch.zeros(MR, N // 2, dtype=torch.bfloat16, device="cuda")
        kw = dict(pro_mode=ops.PRO_RMSNORM, nsplit=0, norm_w=nw, eps=1e-6)
        if "resid" in case:
            kw.update(resid_in=resid)
        if "fx" in case:
            kw.update(fx=fx)
        ops.gemm_fused(None, W, h, ops.fused_args(**kw), epi=ops.EPI_BF16_GELU_MUL | flag, M=M, **nk)
        return (h,)

    check(launch, N, K)


# ---------------------------------------------------------------------------------------------------------- down
@pytest.mark.parametrize("N", [32, 48])
@pytest.mark.parametrize("resid", [False, True])
def test_down_fx_add(N, resid):
    """PG_EPI_FX_ADD, pro_mode 0, K split 2: A and lda in the header (x is a view with a longer row stride), status set,
    resid_in added by split 0 or null."""
    from pghip import ops
    K = 2048
    xw = rnd(MR, K + 64, scale=0.5, seed=21)
    x = xw[:, :K]
    bias = rnd(N, seed=22, dtype=torch.float32)
    res = rnd(MR, N, seed=23, dtype=torch.float32)

    def launch(W, flag, nk, M):
        acc = fx_rows(MR, N, 24)
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        kw = dict(status=st)
        if resid:
            kw.update(resid_in=res)
        ops.gemm_fused(x, W, acc, ops.fused_args(**kw), epi=ops.EPI_FX_ADD | flag, M=M, ksplit=2, bias=bias, **nk)
        assert int(st) == 0
        return (acc,)

    check(launch, N, K)


def test_down_fx_add_reports_overflow_through_status():
    """status reaches the epilogue: a product the accumulator cannot hold sets it (and only then)."""
    from pghip import ops
    N, K = 32, 2048
    for name, W, flag, nk in matrices(N, K):
        for scale, want in ((1.0, 0), (3e38, 1)):
            x = torch.full((1, K), scale, dtype=torch.bfloat16, device="cuda")
            acc = torch.zeros(1, N, dtype=torch.int64, device="cuda")
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.gemm_fused(x, W, acc, ops.fused_args(status=st), epi=ops.EPI_FX_ADD | flag, M=1, ksplit=2, **nk)
            assert int(st) == want, (name, scale)


@pytest.mark.parametrize("N", [32, 48])
@pytest.mark.parametrize("case", ["fx+norm_w", "fx", "resid"])
def test_down_f32_fin(N, case):
    """PG_EPI_F32_FIN, pro_mode 0, K split 2 (the last layer's down): norm_w null (no x' then), the fixed-point
    accumulator folded in and cleared, or the plain residual."""
    from pghip import ops
    K, tiles = 2048, N // 16
    x = rnd(MR, K, scale=0.5, seed=41)
    nw = rnd(N, scale=0.1, seed=42, dtype=torch.float32)
    fx0 = fx_rows(MR, N, 43)

    def launch(W, flag, nk, M):
        part = torch.zeros(2, M, N, device="cuda")
        cnt = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        res = rnd(MR, N, seed=44, dtype=torch.float32)[:M].contiguous()
        ss = torch.zeros(M, tiles, device="cuda")
        xq = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        fx = fx0[:M].clone()
        kw = dict(fin_cnt=cnt, fin_resid=res, ss_out=ss, ss_ld=tiles)
        if "fx" in case:
            kw.update(fx=fx)
        if "norm_w" in case:
            kw.update(fin_x=xq, norm_w=nw)
        ops.gemm_fused(x, W, part, ops.fused_args(**kw), epi=ops.EPI_F32_FIN | flag, M=M, ksplit=2, **nk)
        assert not bool(cnt.any()) and ("fx" not in case or not bool(fx.any()))
        if M <= 4:
            check_ss(ss, res)
        return res, xq

    check(launch, N, K)


# ---------------------------------------------------------------------------------------------------------- lm_head
@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("N", [32, 48])
def test_lm_head_rstd_prologue(N, K):
    """PG_EPI_F32, pro_mode 4: A / lda / ss_in in the header, two tiles per workgroup for the packs (N = 48: the last
    workgroup's second tile is clamped)."""
    from pghip import ops
    xw = rnd(MR, K + 8, seed=51)
    x = xw[:, :K]
    bias = rnd(N, seed=52, dtype=torch.float32)
    n_ss = 64
    g = torch.Generator().manual_seed(53)
    ss_in = torch.randint(1, 4096, (MR, n_ss + 3), generator=g).float().cuda()[:, :n_ss]     # (integers: see the module text)

    def launch(W, flag, nk, M):
        out = torch.zeros(MR, N, device="cuda")
        fa = ops.fused_args(pro_mode=ops.PRO_X_RSTD, ss_in=ss_in, ss_ld=ss_in.stride(0), ss_n=n_ss, eps=1e-6)
        ops.gemm_fused(x, W, out, fa, epi=ops.EPI_F32 | flag, M=M, bias=bias, **nk)
        return (out,)

    check(launch, N, K)


# ---------------------------------------------------------------------------------------------------------- argmax
@pytest.mark.parametrize("V", [257, 4096])
@pytest.mark.parametrize("B", [1, 2])
def test_argmax_embed_pair(V, B):
    """pg_argmax_embed (the partial kernel's struct, the finaliser's reordered parameters) against pg_argmax +
    pg_embed_merge (the same partial kernel, the plain finaliser): a tie at the two
    lowest indices goes to index 0; the same winner, history row, advanced counters and embedded row."""
    from pghip import ops
    H, steps = 64, 4
    logits = rnd(B, (V + 7) // 4 * 4, seed=90, dtype=torch.float32)[:, :V]      # (a row stride above V, % 4 == 0)
    logits[:, 0] = logits[:, 1] = 50.0
    if B > 1:
        logits[1, 0] = logits[1, 1] = -50.0
        logits[1, V - 1] = 60.0
    embed = rnd(V, H, seed=91)
    feat = rnd(4, H, seed=92, dtype=torch.float32)
    outs = []
    for fused in (True, False):
        ids = torch.zeros(B, dtype=torch.int64, device="cuda")
        ws = torch.zeros(B * 64 * 2 + 16, device="cuda")
        hist = torch.full((steps, B), -1, dtype=torch.int64, device="cuda")
        step = torch.tensor([2], dtype=torch.int32, device="cuda")
        pos = torch.tensor([10, 20][:B], dtype=torch.int32, device="cuda")
        kv = torch.tensor([11], dtype=torch.int32, device="cuda")
        res = torch.zeros(B, H, device="cuda")
        kw = dict(image_id=V + 5, pad_id=-1, img_scale=1.0, normalizer=8.0)
        if fused:
            ops.argmax_embed(logits, ids, ws, embed, feat, 4, res, hist=hist, step=step, pos=pos, kv_len=kv, **kw)
        else:
            ops.argmax(logits, ids, ws, hist=hist, step=step, pos=pos, kv_len=kv)
            ops.embed_merge(ids, None, embed, feat, 4, res, **kw)
        torch.cuda.synchronize()
        outs.append((ids, hist, step, pos, kv, res))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    ids, hist, step, pos, kv, res = outs[0]
    assert ids.tolist() == [0, V - 1][:B] and hist[2].tolist() == ids.tolist() and int(step) == 3 and int(kv) == 12
    assert pos.tolist() == [11, 21][:B] and bool(res.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------------------- end to end
E2E_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "karg_hot_tiny8.npz")


def decode_run(B, steps, graph):
    """TINY8 with intermediate 4096 (the config test_frag13_gpu.py uses: every batch-1 GEMV streams a pack), the same
    prompt and image in each of B rows: `steps` greedy tokens, the decode steps replayed from the captured graph or run
    eagerly.  Returns row 0's tokens [steps] and the logits behind each [steps][vocab] (the first from the prefill)."""
    from pghip import configs, engine, synthetic, weights
    cfg = copy.deepcopy(configs.TINY8)
    cfg["text_config"].update(intermediate_size=4096)
    pw = weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__)
    n_img = configs.num_image_tokens(cfg)
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([torch.full((1, n_img), cfg["image_token_index"]), torch.full((1, 1), cfg["bos_token_id"]),
                     torch.randint(3, 290, (1, 6), generator=g)], 1).expand(B, -1).contiguous().cuda()
    px = torch.randn(1, 3, 56, 56, generator=g).expand(B, -1, -1, -1).contiguous().cuda()
    eng = engine.PaliGemmaEngine(cfg, pw)
    V = pw.vocab_local_pad
    cache, feats, logits, nxt = eng.prefill_request(ids, px, torch.ones_like(ids), steps)
    sampler = dict(do_sample=False, temperature=0.8, top_p=0.9)
    st = eng.decode_state(B, cache, nxt, steps, sampler=sampler)
    eng.sample(logits, st, sampler, advance=False, feats=feats)
    rows = [logits.reshape(-1)[:V].clone()]
    step = eng._graph_step(st, cache, feats, sampler) if graph else (lambda: eng.decode_step(st, cache, feats, sampler))
    for _ in range(steps - 1):
        step()
        rows.append(eng._ws["d_logits"][:V].clone())
    torch.cuda.synchronize()
    eng.check_numerics()
    return st["hist"][:steps, 0].cpu().clone(), torch.stack(rows).cpu()


def test_captured_decode_graph_reproduces_the_recorded_tokens_and_logits():
    """6 greedy tokens through the captured batch-1 decode graph -- every hot-header launch of a decode step, replayed:
    the tokens and each step's logits are bit for bit those recorded from the commit before the header
    (tests/golden/karg_hot_tiny8.npz, written by this file's decode_run(1, 6, True) there).
    (Eager decode steps at B = 3, the batched route, are not a bit-exact reference for row 0 -- the batch-1 route adds
    its split-K partials in 2^-32 fixed point, the batched one in fp32 slabs -- on that commit either; the recording says
    by how much they differ, see `b3_max_abs_diff`.)"""
    import numpy as np
    want = np.load(E2E_GOLDEN)
    toks, logits = decode_run(1, 6, True)
    assert toks.tolist() == want["tokens"].tolist()
    assert torch.equal(logits, torch.from_numpy(want["logits"])) and bool(logits.abs().sum() > 0)
    assert np.isfinite(logits.numpy()).all()
