"""The 12-bit form of the exponent-coded weight pack on the device (PG_W_FRAG13 | PG_W_FRAG12): every instantiated GEMV
form launched with the bf16 fragment pack and with the 12-bit pack of the same matrix must give torch.equal outputs.  The
reference is always the PG_W_FRAG launch.  Three matrices per form: every block narrow, every block wide, and a mix in
which the first and last block of a wave's strip (and the blocks either side of a split-2 seam) are wide and blocks with
a zero weight are present.  K picks the kernel path: 2048 and 1024 are the straight-line forms of 8 and 4 chunks per
wave, 512 is one block per wave, 1536 / 3072 run the generic block loop past its ring depth."""
import copy
import functools

import pytest
import torch

from test_frag12_host import block_index, check_boundary_rejections, field
from test_frag13_host import _bits, _random_fields

pytestmark = pytest.mark.gpu

KINDS = ("narrow", "wide", "mixed")


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
    """(row-major bf16 W, its fragment pack, its 12-bit pack) on the device, built once per shape; exponent fields
    around 120 (values near 2^-7) so the products stay in the fixed-point accumulator's range."""
    from pghip.weights import frag_pack, frag12_pack, frag12_table
    T, nb = N // 16, K // 128
    b = _bits(_random_fields((N, K), 112, 124, N + K)).clone()           # span 12: every block narrow
    wide = torch.zeros(T, nb, dtype=torch.bool)
    if kind == "wide":
        far = _bits(_random_fields((N, K), 100, 104, N + K + 1))         # span up to 24, in every block
        sel = (torch.arange(K)[None, :] * 7 + torch.arange(N)[:, None]) % 5 == 0
        b = torch.where(sel, far, b)
        wide[:] = True
    elif kind == "mixed":
        n_i = nb // 4
        for t in range(T):
            w = t % 4
            for i in {0, n_i - 1, max(n_i // 2 - 1, 0), n_i // 2}:       # the strip's ends and the split-2 seam
                r, c = block_index(t, 4 * i + w)
                b[r[15, 0], c[0, 127]] = field(104)                      # (in the block's last element: span >= 22)
                b[r[0, 0], c[0, 0]] = field(126)
                wide[t, 4 * i + w] = True
            z = 4 * (n_i // 2) + (t + 1) % 4                             # a block with zero weights, on another wave
            r, c = block_index(t, z)
            b[r[3, 0], c[0, 40]], b[r[9, 0], c[0, 100]] = 0, -32768
            wide[t, z] = True
    w = b.view(torch.bfloat16).cuda()
    p12 = frag12_pack(w)
    assert p12 is not None, (kind, N, K)
    _, zflag, wd, _, _ = frag12_table(p12.cpu(), N, K)
    assert torch.equal(wd.bool(), wide), (kind, N, K)
    assert kind != "mixed" or int(zflag.sum()) == T
    return w, frag_pack(w), p12


def both(launch, kind, N, K):
    """launch(W, layout flag, N / K keywords) -> tensors; run with the fragment pack, then the 12-bit pack; all equal."""
    from pghip import ops
    _, wf, w12 = weights_of(kind, N, K)
    want = launch(wf, ops.W_FRAG, {})
    got = launch(w12, ops.W_FRAG13 | ops.W_FRAG12, dict(N=N, K=K))
    torch.cuda.synchronize()
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (i, kind, N, K)
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("K", [2048, 1024, 512, 3072])
def test_qkv_rope_rmsnorm_prologue(M, K, kind):
    """PG_EPI_QKV_ROPE, pro_mode 1, one tile per workgroup: q rows and all four cache layouts."""
    from pghip import engine, ops
    hd, nh, nkv, Smax = 16, 1, 1, 32
    N = (nh + 2 * nkv) * hd                                # 48: three tiles
    cos_t, sin_t = engine.rope_tables(hd, 64, 10000.0, "cuda")
    resid = rnd(M, K, seed=1, dtype=torch.float32)
    nw = rnd(K, scale=0.1, seed=2, dtype=torch.float32)
    pos = torch.tensor([5, 9][:M], dtype=torch.int32, device="cuda")
    slot = torch.tensor([3], dtype=torch.int32, device="cuda")

    def launch(W, flag, nk):
        kc, vtc = rnd(M, Smax, nkv * hd, seed=3), rnd(M, nkv * hd, Smax, seed=4)
        kd, vd = rnd(M * Smax * nkv * hd, seed=5), rnd(M * Smax * nkv * hd, seed=6)
        q = torch.zeros(M, nh * hd, dtype=torch.bfloat16, device="cuda")
        fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, resid_in=resid, nsplit=0, norm_w=nw, eps=1e-6, head_dim=hd,
                            cos_t=cos_t, sin_t=sin_t, pos=pos, rows_per_batch=1, kc=kc, vtc=vtc, kd=kd, vd=vd,
                            smax=Smax, q_heads=nh, kv_heads=nkv, slot_dev=slot, slot_base=0)
        ops.gemm_fused(None, W, q, fa, epi=ops.EPI_QKV_ROPE | flag, M=M, **nk)
        return q, kc, vtc, kd, vd

    q = both(launch, kind, N, K)[0]
    assert bool(q.float().abs().sum() > 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("K", [2048, 1024, 512, 1536])
def test_gate_up_rmsnorm_prologue(M, K, kind):
    """PG_EPI_BF16_GELU_MUL, pro_mode 1, the interleaved gate/up tile pair per workgroup (three pairs)."""
    from pghip import ops
    N = 96
    resid = rnd(M, K, seed=11, dtype=torch.float32)
    nw = rnd(K, scale=0.1, seed=12, dtype=torch.float32)

    def launch(W, flag, nk):
        h = torch.zeros(M, N // 2, dtype=torch.bfloat16, device="cuda")
        fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, resid_in=resid, nsplit=0, norm_w=nw, eps=1e-6)
        ops.gemm_fused(None, W, h, fa, epi=ops.EPI_BF16_GELU_MUL | flag, M=M, **nk)
        return (h,)

    h = both(launch, kind, N, K)[0]
    assert bool(h.float().abs().sum() > 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K,ks", [(48, 2048, 1), (48, 2048, 2), (48, 512, 1), (48, 1024, 2), (48, 3072, 1)])
def test_fx_add_plain_rows(M, N, K, ks, kind):
    """PG_EPI_FX_ADD, pro_mode 0 (down): the fixed-point accumulator after the launch, bias by split 0."""
    from pghip import ops
    x = rnd(M, K, scale=0.5, seed=21)
    bias = rnd(N, seed=22, dtype=torch.float32)

    def launch(W, flag, nk):
        acc = torch.full((M, N), 12345, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.gemm_fused(x, W, acc, ops.fused_args(status=st), epi=ops.EPI_FX_ADD | flag, M=M, ksplit=ks, bias=bias,
                       **nk)
        return acc, st

    acc, st = both(launch, kind, N, K)
    assert int(st) == 0 and bool((acc != 12345).any())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("ks", [1, 2])
def test_fx_add_attention_merge_prologue(M, ks, kind):
    """PG_EPI_FX_ADD, pro_mode 2 (o_proj): x merged from split-KV partials in the prologue."""
    from pghip import ops
    nh, nkv, hd, S, dt = 8, 1, 256, 4, 256
    N, K = 48, nh * hd
    po = rnd(M * nkv * S * 16 * dt, seed=31, dtype=torch.float32)
    ml = torch.stack([rnd(M * nkv * S * 16, seed=32, dtype=torch.float32),
                      rnd(M * nkv * S * 16, seed=33, dtype=torch.float32).abs() + 0.5], -1).contiguous()

    def launch(W, flag, nk):
        acc = torch.zeros(M, N, dtype=torch.int64, device="cuda")
        fa = ops.fused_args(pro_mode=ops.PRO_ATTN_COMBINE, part_o=po, part_ml=ml, asplit=S, head_dim=hd, dtw=dt,
                            q_per_kv=nh // nkv, kv_heads=nkv)
        ops.gemm_fused(None, W, acc, fa, epi=ops.EPI_FX_ADD | flag, M=M, ksplit=ks, **nk)
        return (acc,)

    assert bool((both(launch, kind, N, K)[0] != 0).any())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K,ks", [(48, 2048, 1), (48, 2048, 2), (48, 512, 1), (48, 3072, 1)])
def test_f32_fin_last_down(M, N, K, ks, kind):
    """PG_EPI_F32_FIN, pro_mode 0 (the last layer's down): finalised residual, x', sums of squares, cleared tickets and
    the fixed-point accumulator it folds in and clears."""
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(80, 2048), (96, 1024), (80, 512), (80, 1536)])   # 80: the last second tile is clamped
def test_lm_head_rstd_prologue(M, N, K, kind):
    """PG_EPI_F32, pro_mode 4, two tiles per workgroup (the lm_head): logits with bias, scaled by the row's rstd."""
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


def test_12bit_result_against_fp64_matmul():
    """The pairs above compare two kernels: anchor the shared result once against torch (fp64)."""
    from pghip import ops
    M, N, K = 2, 48, 2048
    w, _, w12 = weights_of("mixed", N, K)
    x = rnd(M, K, scale=0.5, seed=61)
    acc = torch.zeros(M, N, dtype=torch.int64, device="cuda")
    ops.gemm_fused(x, w12, acc, ops.fused_args(), epi=ops.EPI_FX_ADD | ops.W_FRAG13 | ops.W_FRAG12, M=M, ksplit=2, N=N,
                   K=K)
    got = acc.double() / 2.0 ** 32
    want = x.double() @ w.double().t()
    # K products of bf16 values summed in fp32 and rounded to 2^-32 fixed point: 2^-20 of the row's absolute sum is ample
    bound = (x.double().abs() @ w.double().abs().t()) * 2.0 ** -20 + 2.0 ** -30
    assert bool(((got - want).abs() <= bound).all())


def test_boundary_rejections_on_the_device_build():
    check_boundary_rejections()


def test_ops_rejects_a_pack_of_the_wrong_form():
    from pghip import ops
    from pghip.weights import frag13_pack
    w, _, w12 = weights_of("narrow", 48, 2048)
    acc = torch.zeros(1, 48, dtype=torch.int64, device="cuda")
    x = rnd(1, 2048, seed=71)
    with pytest.raises(ValueError):
        ops.gemm_fused(x, w12, acc, ops.fused_args(), epi=ops.EPI_FX_ADD | ops.W_FRAG13, M=1, N=48, K=2048)
    with pytest.raises(ValueError):
        ops.gemm_fused(x, frag13_pack(w), acc, ops.fused_args(), epi=ops.EPI_FX_ADD | ops.W_FRAG13 | ops.W_FRAG12, M=1,
                       N=48, K=2048)


@pytest.mark.parametrize("B", [1, 2])
def test_decode_steps_bit_equal_with_the_12bit_and_the_13bit_pack(B, monkeypatch):
    """8 greedy decode steps with the weights held in the 12-bit form (w12 on) and in the 13-bit form (off): the same
    token ids and bit-equal logits at every step; neither PackedWeights holds a matrix in both forms.  The config is
    TINY8 with the intermediate size raised to 4096, the smallest whose every decode launch has whole blocks."""
    from pghip import configs, engine, synthetic, weights
    cfg = copy.deepcopy(configs.TINY8)
    cfg["text_config"].update(intermediate_size=4096)
    sd = synthetic.SyntheticStateDict(cfg)
    n_img = configs.num_image_tokens(cfg)
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([torch.full((B, n_img), cfg["image_token_index"]), torch.full((B, 1), cfg["bos_token_id"]),
                     torch.randint(3, 290, (B, 6), generator=g)], 1).cuda()
    px = torch.randn(B, 3, 56, 56, generator=g).cuda()
    mask = torch.ones_like(ids)
    outs = []
    real = engine.ops.gemm_fused
    for on in (True, False):
        pw = weights.PackedWeights(cfg, sd.__getitem__, w12=on)
        forms = weights.W12_FORMS if on else ()
        assert pw.w12_forms == forms
        T = {"gu": pw.tl[0]["gu_w"].shape, "down": pw.tl[0]["down_w"].shape, "lm": pw.lm_w.shape}
        for name, (n, k) in T.items():
            p = pw.lm_w13 if name == "lm" else pw.tl[0][name + "_w13"]
            is12 = p.numel() != weights.frag13_size(n, k)
            assert is12 == (name in forms), (name, on)          # one form per matrix: the key holds one tensor
            assert not any(key.endswith("_w12") for key in pw.tl[0])
        eng = engine.PaliGemmaEngine(cfg, pw)
        flags, logits = [], []

        def recording(*a, **kw):
            flags.append(kw.get("epi", 0) & (engine.ops.W_FRAG13 | engine.ops.W_FRAG12))
            out = real(*a, **kw)
            if (kw.get("epi", 0) & 0xFF) == engine.ops.EPI_F32 and kw.get("M") == B and a[2].shape[-1] == \
                    pw.vocab_local_pad:
                logits.append(a[2].clone())                                  # the step's logits
            return out

        monkeypatch.setattr(engine.ops, "gemm_fused", recording)
        toks = eng.generate(ids, px, mask, 8, stop_token=None, use_graph=False)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine.ops, "gemm_fused", real)
        n12 = sum(f == (engine.ops.W_FRAG13 | engine.ops.W_FRAG12) for f in flags)
        n13 = sum(f == engine.ops.W_FRAG13 for f in flags)
        # per step: gate/up and down per layer and the lm_head stream a pack (W13_FORMS), those in `forms` the 12-bit one
        assert eng.W13_FORMS == ("gu", "down", "lm")
        per12 = sum(n in forms for n in ("gu", "down")) * pw.t_layers + ("lm" in forms)
        per13 = 2 * pw.t_layers + 1 - per12
        if on:
            assert per12 > 0 and n12 >= 7 * per12 and n12 % per12 == 0 and n13 * per12 == n12 * per13, (n12, n13)
        else:
            assert n12 == 0 and n13 >= 7 * per13 and n13 % per13 == 0, (n12, n13)
        assert not any(f == engine.ops.W_FRAG12 for f in flags)
        outs.append((torch.as_tensor(toks).clone(), logits))
    assert torch.equal(outs[0][0], outs[1][0])
    assert len(outs[0][1]) == len(outs[1][1]) >= 7
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b) and bool(a.abs().sum() > 0)
