"""The 13-bit weight pack on the device (PG_W_FRAG13): every instantiated GEMV form launched with the bf16 fragment
pack and with its 13-bit pack must give torch.equal outputs -- the kernel rebuilds the PG_W_FRAG operands bit for bit
and runs them in the same order.  The reference is always the PG_W_FRAG launch.  Accumulating forms use the fixed-point
(order-independent) PG_EPI_FX_ADD the engine uses."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import synth
from test_frag13_host import _bf16_from_fields, _random_fields, check_boundary_rejections

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


KINDS = ("synth", "zeros", "ends")


@functools.lru_cache(maxsize=None)
def weights_of(kind: str, N: int, K: int):
    """(row-major bf16 W, its fragment pack, its 13-bit pack) on the device, built once per shape.
    synth: the oracle's synthetic recipe; zeros: the same with planted +-0, denormals and a whole zero tile row range;
    ends: tile 0's blocks hold both ends of the code range (exponent fields base and base + 30)."""
    from pghip.weights import frag_pack, frag13_pack
    w = torch.from_numpy(synth.generate(f"frag13.{kind}.{N}x{K}.weight", (N, K))).bfloat16()
    b = w.view(torch.int16)
    if kind == "zeros":
        g = torch.Generator().manual_seed(N + K)
        idx = torch.randint(0, N * K, (max(64, N * K // 97),), generator=g)
        vals = torch.tensor([0, -32768, 1, 0x7F, -32768 + 5, 0x40], dtype=torch.int16)   # +-0 and bf16 denormals
        b.view(-1)[idx] = vals[torch.arange(idx.numel()) % vals.numel()]
        b[8:12, :] = 0                                  # four zero rows inside tile 0
    elif kind == "ends":
        lo = _random_fields((16, K), 96, 96, 7).view(torch.int16)
        hi = _random_fields((16, K), 126, 126, 8).view(torch.int16)
        mid = _random_fields((16, K), 96, 126, 9).view(torch.int16)
        sel = (torch.arange(K)[None, :] + torch.arange(16)[:, None]) % 3
        b[:16] = torch.where(sel == 0, lo, torch.where(sel == 1, hi, mid))
    w = w.cuda()
    p13 = frag13_pack(w)
    assert p13 is not None, (kind, N, K)
    return w, frag_pack(w), p13


def both(launch, kind, N, K):
    """launch(W, layout flag, N / K keywords) -> tensors; run with the fragment pack, then the 13-bit pack; all equal."""
    from pghip import ops
    _, wf, w13 = weights_of(kind, N, K)
    want = launch(wf, ops.W_FRAG, {})
    got = launch(w13, ops.W_FRAG13, dict(N=N, K=K))
    torch.cuda.synchronize()
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (i, kind, N, K)
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("K", [2048, 1024])            # ksplit is 1 here: 8 and 4 chunks per wave
def test_qkv_rope_rmsnorm_prologue(M, K, kind):
    """PG_EPI_QKV_ROPE, pro_mode 1, one tile per workgroup: q rows and all four cache layouts."""
    from pghip import engine, ops
    hd, nh, nkv, Smax = 16, 1, 1, 32
    N = (nh + 2 * nkv) * hd                                # 48: three tiles
    cos_t, sin_t = engine.rope_tables(hd, 64, 10000.0, "cuda")
    resid = rnd(M, K, seed=1, dtype=torch.float32)
    nw = rnd(K, scale=0.1, seed=2, dtype=torch.float32)
    pos = torch.tensor([5, 9, 2, 30][:M], dtype=torch.int32, device="cuda")
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
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("K", [2048, 1024])
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
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("N,K,ks", [(48, 2048, 1), (48, 2048, 2),      # 8 and 4 chunks per wave
                                    (48, 2048, 4),                     # 2: the generic block loop
                                    (16, 16384, 8)])                   # the down projection's shape
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
@pytest.mark.parametrize("M", [1, 2, 4])
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
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("N,K,ks", [(48, 2048, 1), (48, 2048, 2), (16, 16384, 8)])
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
@pytest.mark.parametrize("M", [1, 2])                  # (pro_mode 4 at one tile pair per workgroup takes at most 2 rows)
@pytest.mark.parametrize("N,K", [(80, 2048), (96, 1024)])   # five tiles: the last workgroup's second tile is clamped
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


def test_13bit_result_against_fp32_matmul():
    """The pair above only compares two kernels: anchor the shared result once against torch (fp32 accumulate)."""
    from pghip import ops
    M, N, K = 2, 48, 2048
    w, _, w13 = weights_of("synth", N, K)
    x = rnd(M, K, scale=0.5, seed=61)
    acc = torch.zeros(M, N, dtype=torch.int64, device="cuda")
    ops.gemm_fused(x, w13, acc, ops.fused_args(), epi=ops.EPI_FX_ADD | ops.W_FRAG13, M=M, ksplit=2, N=N, K=K)
    got = acc.double() / 2.0 ** 32
    want = x.double() @ w.double().t()
    # K products of bf16 values summed in fp32 and rounded to 2^-32 fixed point: 2^-20 of the row's absolute sum is ample
    bound = (x.double().abs() @ w.double().abs().t()) * 2.0 ** -20 + 2.0 ** -30
    assert bool(((got - want).abs() <= bound).all())


def test_matrix_that_does_not_pack_decodes_from_the_fragment_pack():
    """A block spanning 32 exponent fields has no 13-bit pack: the engine's per-launch choice is the PG_W_FRAG tensor
    and flag, and the launch gives what it gave before."""
    from pghip import engine, ops
    from pghip.weights import frag_pack, frag13_pack
    M, N, K = 1, 16, 2048
    w = _random_fields((N, K), 100, 120, 70)
    w.view(torch.int16)[3, 17] = (89 << 7) | 3               # fields 89 .. 120 in one block
    w = w.cuda()
    assert frag13_pack(w) is None
    eng = SimpleNamespace(W13=True, W13_FORMS=engine.PaliGemmaEngine.W13_FORMS, FUSE_MAX_B=2, tp=1,
                          w=SimpleNamespace(wflag=ops.W_FRAG))
    d = {"down_w": frag_pack(w)}
    W, flag, nk = engine.PaliGemmaEngine._dec_w(eng, d, "down", M, 2)
    assert W is d["down_w"] and flag == ops.W_FRAG and nk == {}
    # ... and a matrix that packs is taken only where the split leaves every wave whole blocks
    _, wf, w13 = weights_of("synth", 48, 2048)
    d = {"down_w": wf, "down_w13": w13}
    assert engine.PaliGemmaEngine._dec_w(eng, d, "down", M, 2)[1] == ops.W_FRAG13
    assert engine.PaliGemmaEngine._dec_w(eng, d, "down", M, 8)[1] == ops.W_FRAG        # 4 chunks per split
    assert engine.PaliGemmaEngine._dec_w(eng, d, "down", 3, 2)[1] == ops.W_FRAG        # above FUSE_MAX_B
    x = rnd(M, K, seed=71)
    a, b = (torch.zeros(M, N, dtype=torch.int64, device="cuda") for _ in range(2))
    ops.gemm_fused(x, W, a, ops.fused_args(), epi=ops.EPI_FX_ADD | flag, M=M, ksplit=2, **nk)
    ops.gemm_fused(x, frag_pack(w), b, ops.fused_args(), epi=ops.EPI_FX_ADD | ops.W_FRAG, M=M, ksplit=2)
    assert torch.equal(a, b) and bool(a.any())


def test_boundary_rejections_on_the_device_build():
    check_boundary_rejections()


@pytest.mark.parametrize("B", [1, 2])
def test_decode_steps_bit_equal_with_and_without_the_pack(B, monkeypatch):
    """8 greedy decode steps with the 13-bit launches on and off: the same token ids and bit-equal final logits.  The
    config is the suite's TINY8 (hidden 1024 = 8 x 128 q heads: o_proj K 1024 at split 2) with the intermediate size
    raised to 4096, the smallest at which the split-8 down projection leaves every wave whole 128-k blocks."""
    import copy
    from pghip import configs, engine, synthetic, weights
    cfg = copy.deepcopy(configs.TINY8)
    cfg["text_config"].update(intermediate_size=4096)
    sd = synthetic.SyntheticStateDict(cfg)
    pw = weights.PackedWeights(cfg, sd.__getitem__)
    assert pw.lm_w13 is not None and all(k + "_w13" in L for L in pw.tl for k in ("qkv", "o", "gu", "down"))
    n_img = configs.num_image_tokens(cfg)
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([torch.full((B, n_img), cfg["image_token_index"]), torch.full((B, 1), cfg["bos_token_id"]),
                     torch.randint(3, 290, (B, 6), generator=g)], 1).cuda()
    px = torch.randn(B, 3, 56, 56, generator=g).cuda()
    mask = torch.ones_like(ids)
    outs = []
    real = engine.ops.gemm_fused
    for on in (True, False):
        eng = engine.PaliGemmaEngine(cfg, pw)
        eng.W13 = on
        packed = []

        def counting(*a, **kw):
            packed.append(bool(kw.get("epi", 0) & engine.ops.W_FRAG13))
            return real(*a, **kw)

        monkeypatch.setattr(engine.ops, "gemm_fused", counting)
        toks = eng.generate(ids, px, mask, 8, stop_token=None, use_graph=False)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine.ops, "gemm_fused", real)
        logits = eng._ws["d_logits"][:B * pw.vocab_local_pad].clone()      # the last step's logits
        # on: every decode step's GEMVs of the forms the engine keeps (W13_FORMS) stream the pack; off: no launch does
        forms = eng.W13_FORMS
        n13 = sum(packed)
        per_step = sum(n in forms for n in ("qkv", "o", "gu", "down")) * pw.t_layers + ("lm" in forms)
        assert (n13 >= 7 * per_step and n13 % per_step == 0) if on else n13 == 0, (on, n13)
        outs.append((torch.as_tensor(toks).clone(), logits))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and bool(outs[0][1].abs().sum() > 0)
