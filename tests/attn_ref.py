"""Float64 reference, structured inputs and the error bound for the attention kernels
(tests/test_attn_structured_gpu.py; checked on the host by tests/test_attn_ref_host.py).

Plain torch, no project imports.  Gaussian q / k / v give a diffuse softmax over a narrow logit band: a key dropped,
counted twice or admitted from beyond the length moves the output by |v| / L, below any bound on the scaled max error
from about 64 keys on.  The inputs here make one key matter:

  census  q = 0, v one-hot in d = key % D: every weight is exactly 1 and o[d] = count_d / L, so one key too many or too
          few changes a count by one
  needle  k random signs, q = c k[needle]: one key holds > 0.99 of a row's weight, every key is some row's needle
  ramp    logits rising (the running max moves in every block) or falling (it never moves after block 0) over +-20..50
  spike   the falling ramp plus one key far above everything: all that was accumulated before it underflows

Shapes: q [B][nh][Lq][D], k / v [B][nkv][Smax][D], float32 holding bf16-representable values; row b attends its first
lens[b] keys and the cache rows past that hold finite poison (k random, v = +64 in every dimension), so one stale key
admitted shows in every output element.
"""
import math

import torch

POISON_V = 64.0

# The bound on needle / ramp / spike (and masked Gaussian) outputs, per element:
#     |o - ref| <= C * budget + 1e-30,    budget = sum_j p_j |v_jd|
# C is twice the worst |o - ref| / budget of emulate() below -- fp32 logits, online softmax over 32- or 64-key blocks,
# P rounded to bf16, fp32 sums, o rounded to bf16 -- over every builder at D in {32, 72, 256}, L in {100, 264, 1000},
# both block sizes (tests/test_attn_ref_host.py asserts worst <= C / 2), rounded up to a power of two.  The factor 2
# covers the hardware exp2 and another summation order.  Measured worst ratio: 1.337 * 2^-8 (ramp, D = 256, L = 100,
# where a handful of keys share the weight: each P and the output round to bf16 once); needle 0.84 * 2^-8 at most.
EMU_WORST = 1.337 * 2.0 ** -8
C = 2.0 ** -6                # = 2 * EMU_WORST = 2.67 * 2^-8, rounded up to a power of two
CENSUS_RTOL = 2.0 ** -7      # census: one bf16 ulp of the exact count_d / L (a reciprocal in place of the division)


def bf16_exact(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _logits64(q, k, scale, b, n):
    """fp64 logits of batch row b over its first n keys: [nh][Lq][n]."""
    g = q.shape[1] // k.shape[1]
    kb = k[b, :, :n].double().repeat_interleave(g, 0)
    return (q[b].double() @ kb.transpose(-1, -2)) * scale


def ref(q, k, v, scale, mask=None, lens=None):
    """fp64 softmax attention, one batch row at a time on the inputs' device, GQA by repeat_interleave.
    mask: additive, broadcastable to [B][nh][Lq][keys]; lens: keys row b attends (default: all of k).
    Returns (o, budget) fp64 [B][nh][Lq][D] with budget = softmax @ |v|."""
    B, nh = q.shape[0], q.shape[1]
    g = nh // k.shape[1]
    os_, bs_ = [], []
    for b in range(B):
        n = k.shape[2] if lens is None else int(lens[b])
        s = _logits64(q, k, scale, b, n)
        if mask is not None:
            mb = mask[b if mask.shape[0] > 1 else 0]
            s = s + mb[..., :n].double()
        p = torch.softmax(s, -1)
        vb = v[b, :, :n].double().repeat_interleave(g, 0)
        os_.append(p @ vb)
        bs_.append(p @ vb.abs())
    return torch.stack(os_), torch.stack(bs_)


def emulate(q, k, v, scale, block):
    """What a flash kernel computes, on the CPU: fp32 logits (log2 domain), online softmax over `block`-key blocks,
    P rounded to bf16 for P.V, fp32 sums, o rounded to bf16.  k / v hold exactly the keys attended."""
    B, nh, Lq, D = q.shape
    g = nh // k.shape[1]
    kf = k.float().repeat_interleave(g, 1)
    vf = v.float().repeat_interleave(g, 1)
    s = (q.float() @ kf.transpose(-1, -2)) * torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    m = torch.full((B, nh, Lq, 1), float("-inf"))
    l = torch.zeros(B, nh, Lq, 1)
    o = torch.zeros(B, nh, Lq, D)
    for k0 in range(0, kf.shape[2], block):
        x = s[..., k0:k0 + block]
        mn = torch.maximum(m, x.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - mn)
        p = torch.exp2(x - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + bf16_exact(p) @ vf[:, :, k0:k0 + block]
        m = mn
    return bf16_exact(o / l)


def worst_ratio(o, ref_o, budget) -> float:
    """max |o - ref| / budget over the elements (budget is > 0 wherever v is not all zero)."""
    d = (o.double() - ref_o).abs()
    return float((d / budget.clamp_min(1e-300)).max())


def within(o, ref_o, budget, c=None) -> bool:
    c = C if c is None else c
    return bool(((o.double() - ref_o).abs() <= c * budget + 1e-30).all())


def _poison(k, v, lens, seed):
    """Rows past each length: k random, v = +64."""
    gk = _gen(seed + 7919)
    for b, n in enumerate(lens):
        if n < k.shape[2]:
            k[b, :, n:] = bf16_exact(torch.randn(k.shape[1], k.shape[2] - n, k.shape[3], generator=gk))
            v[b, :, n:] = POISON_V
    return k, v


def _finish(q, k, v, device):
    for t in (q, k, v):
        assert torch.equal(t, bf16_exact(t)), "inputs must be exactly representable in bf16"
    return q.to(device), k.to(device), v.to(device)


def census(B, nh, nkv, Lq, D, Smax, lens, seed=0, device="cpu"):
    """q = 0, v[key][d] = 1 if d == key % D else 0, k random: every logit 0, every weight exactly 1, l = len_b exactly,
    every fp32 accumulator a small integer; o[d] = count_d / len_b (census_expected)."""
    for n in lens:
        assert 1 <= n <= Smax and -(-n // D) <= 32, "one key must move an output by >= 4 x the bound: ceil(L / D) <= 32"
    q = torch.zeros(B, nh, Lq, D)
    k = bf16_exact(torch.randn(B, nkv, Smax, D, generator=_gen(seed)))
    v = torch.zeros(B, nkv, Smax, D)
    key = torch.arange(Smax)
    v[:, :, key, key % D] = 1.0
    k, v = _poison(k, v, lens, seed)
    return _finish(q, k, v, device)


def census_expected(D, n):
    """count_d / n for d < D, fp64: the exact census output of a row attending n keys."""
    d = torch.arange(D)
    cnt = (n - d + D - 1).clamp_min(0) // D           # keys j < n with j % D == d
    return cnt.double() / n


def census_ok(o, D, lens) -> bool:
    """|o - count_d / len_b| <= 2^-7 count_d / len_b for every (b, head, row)."""
    for b, n in enumerate(lens):
        e = census_expected(D, n).to(o.device)
        if not bool(((o[b].double() - e).abs() <= CENSUS_RTOL * e).all()):
            return False
    return True


def needle_gain(D) -> float:
    """c of q = c k[needle]: the needle's logit is c sqrt(D), the others' c N(0, 1); the mean weight off the needle is
    about L exp(c^2 / 2 - c sqrt(D)).  32 / sqrt(D) puts the needle at logit 32 (c = 2 at D = 256); sqrt(D) is the best
    any c does, and is taken for the small head_dims (D < 32).  Rounded to a multiple of 1/8: c * (+-1) is bf16-exact.
    D < 24 (head_dim 16): among a few hundred rows of random signs some key agrees with a needle in all dims but one
    (D 2^-D per pair), and its logit is only 2 c / sqrt(D) below the needle's whatever the spread of the others, so
    there the gain is 4 sqrt(D): that key sits 8 below, the needle at logit 4 D = 64."""
    if D < 24:
        return round(4.0 * math.sqrt(D) * 8) / 8
    return round(min(32.0 / math.sqrt(D), math.sqrt(D)) * 8) / 8


def needle(B, nh, nkv, Lq, D, Smax, lens, seed=0, needles=None, device="cpu"):
    """k random signs, v Gaussian, q[row] = c k[needle(row)].  Prefill (needles None): row i of (b, head) takes
    perm_{b,head}(i mod len_b) over the row's own len_b keys, so every key is some row's needle (Lq >= len_b).
    Decode (Lq == 1): needles int [B][nkv], one key per (batch row, kv head) shared by its query heads (edge_fills).
    Asserts the needle's fp64 softmax weight > 0.99 for every row."""
    gq = _gen(seed)
    k = torch.randint(0, 2, (B, nkv, Smax, D), generator=gq).float() * 2 - 1
    v = bf16_exact(torch.randn(B, nkv, Smax, D, generator=gq))
    c = needle_gain(D)
    g = nh // nkv
    idx = torch.empty(B, nh, Lq, dtype=torch.long)
    for b, n in enumerate(lens):
        for h in range(nh):
            if needles is None:
                perm = torch.randperm(n, generator=gq)
                idx[b, h] = perm[torch.arange(Lq) % n]
            else:
                assert Lq == 1 and 0 <= int(needles[b][h // g]) < n
                idx[b, h] = int(needles[b][h // g])
    kq = k.repeat_interleave(g, 1)                                           # [B][nh][Smax][D]
    q = c * torch.gather(kq, 2, idx[..., None].expand(B, nh, Lq, D))
    k, v = _poison(k, v, lens, seed)
    q, k, v = _finish(q, k, v, device)
    idx = idx.to(device)
    for b, n in enumerate(lens):
        p = torch.softmax(_logits64(q, k, D ** -0.5, b, n), -1)
        w = torch.gather(p, 2, idx[b][..., None])
        assert float(w.min()) > 0.99, f"needle weight {float(w.min()):.4f} (D={D}, len={n})"
    return q, k, v


def edge_fills(edges, B, nkv, lens):
    """The decode needles: the (batch row, kv head) pairs walk `edges` cyclically, fill f starting B * nkv further on,
    over ceil(len(edges) / (B * nkv)) fills, so every edge is some pair's needle.  An edge at or past a row's own
    length is clamped to the row's last key.  Returns a list of int lists [B][nkv]."""
    edges = sorted(set(int(e) for e in edges if e >= 0))
    per = B * nkv
    fills = []
    for f in range(-(-len(edges) // per)):
        fills.append([[min(edges[(f * per + b * nkv + h) % len(edges)], int(lens[b]) - 1) for h in range(nkv)]
                      for b in range(B)])
    return fills


RAMP_LOGIT = 32.0     # the largest main-term |logit| of a ramp; the noise terms add a few units
SPIKE_GAIN = 6.0      # spike key = SPIKE_GAIN * u: its logit is 6 x the ramp's top for the same query row


def ramp(B, nh, nkv, Lq, D, Smax, lens, seed=0, down=False, spike=None, device="cpu"):
    """k[key] = a_key u + 0.25 noise, q[row] = g_row u + 0.1 noise, u a fixed sign vector, v Gaussian.  a runs linearly
    over the row's own keys from -1 to 1 (up) or 1 to -1 (down); the gains g_row lie in [0.8, 1] * 32 / sqrt(D), so the
    largest |logit| is about 32 plus the noise term 0.25 g N(0, 1): asserted within [20, 50].
    spike (int [B], with down): that key becomes SPIKE_GAIN * u, asserted >= 60 above every other logit of every row."""
    gq = _gen(seed)
    u = torch.randint(0, 2, (D,), generator=gq).float() * 2 - 1
    gmax = RAMP_LOGIT / math.sqrt(D)
    k = 0.25 * torch.randn(B, nkv, Smax, D, generator=gq)
    for b, n in enumerate(lens):
        a = torch.linspace(-1.0, 1.0, n) if n > 1 else torch.ones(1)
        k[b, :, :n] += (a.flip(0) if down else a)[None, :, None] * u
        if spike is not None:
            assert down and 0 <= int(spike[b]) < n
            k[b, :, int(spike[b])] = SPIKE_GAIN * u
    i = torch.arange(Lq)[None, None, :]
    h = torch.arange(nh)[None, :, None]
    bb = torch.arange(B)[:, None, None]
    gain = gmax * (0.8 + 0.02 * ((7 * i + 3 * h + 5 * bb) % 11))              # [B][nh][Lq]
    q = gain[..., None] * u + 0.1 * torch.randn(B, nh, Lq, D, generator=gq)
    v = bf16_exact(torch.randn(B, nkv, Smax, D, generator=gq))
    q, k = bf16_exact(q), bf16_exact(k)
    k, v = _poison(k, v, lens, seed)
    q, k, v = _finish(q, k, v, device)
    for b, n in enumerate(lens):
        s = _logits64(q, k, D ** -0.5, b, n)
        if spike is None:
            assert 20 <= float(s.abs().max()) <= 50, f"largest |logit| {float(s.abs().max()):.1f}"
        else:
            sp = int(spike[b])
            rest = torch.cat([s[..., :sp], s[..., sp + 1:]], -1)
            if rest.shape[-1]:
                margin = float((s[..., sp] - rest.max(-1).values).min())
                assert margin >= 60, f"spike margin {margin:.1f}"
    return q, k, v
