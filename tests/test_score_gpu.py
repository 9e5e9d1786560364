"""Scoring given answers: prefix-LM prefill attention (pg_attention_prefix), token log-probabilities
(pg_token_logprob) and PaliGemmaEngine.score / PaliGemmaForConditionalGeneration.score.

The rule under test: batch row b's query at position p attends key j iff j < vis_b(p) = min(len_b, max(prefix_b,
p + 1)).  Bounds are the project's existing ones: kernel outputs against fp32 torch < 2e-2 (test_ragged_gpu.KTOL, its
scaled max error), logits < 3e-2 (TOL), an fp32 softmax 1e-4 (test_attn_structured_gpu.PROBS_RTOL), the census 2^-7
(attn_ref.CENSUS_RTOL).  A log-probability moves by at most 2 delta when every logit moves by at most delta (the
target's logit by delta, the log-sum-exp by delta), so log-probs are bounded by 2 * TOL * max |reference logits|.
The engine references live in tests/ragged_ref.py and tests/score_ref.py (computed once, shared)."""
import numpy as np
import pytest
import torch

import attn_ref as A
import ragged_ref as R
import score_ref as S
from test_attn_structured_gpu import PROBS_RTOL, _heads, _layout
from test_ragged_gpu import KTOL, TOL, err, i32, nerr, ragged_lens, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------ 1. prefix-LM attention
# the shape lists of test_ragged_gpu: small shapes, the flash forms (key splits included), the fallback kernels
SMALL = [(4, 150, 4, 1, 32, 0, False), (4, 150, 8, 2, 72, 0, False), (4, 150, 8, 2, 128, 0, False),
         (4, 150, 8, 1, 256, 0, False), (5, 200, 8, 4, 256, 0, False), (8, 600, 8, 8, 32, 0, False)]
FLASH = [(14, 300, 8, 1, 256, 0, False), (16, 1032, 8, 1, 256, 0, False), (32, 1000, 8, 1, 256, 0, False),
         (4, 264, 8, 1, 256, 5, False), (2, 200, 4, 2, 64, 8, False), (1, 264, 8, 1, 256, 5, False)]
# Key splits whose workgroups span more positions than a key block holds keys: 8 waves (128 rows) at G = 1 are 128
# positions on 64-key blocks, so the rows of a workgroup's first half cannot see into the last block it walks.  In the
# key-split shapes above a workgroup covers at most 32 positions that start on a multiple of 32: its walk ends in the
# block its first row already sees into, and every split a row cannot see holds no block at all (blind_rows == 0).
BLIND = [(8, 600, 8, 8, 32, 4, False), (8, 300, 16, 16, 72, 4, False)]
FALLBACK = [(4, 150, 8, 1, 256, 0, True), (3, 150, 4, 2, 72, 0, True), (8, 300, 8, 1, 32, 0, True)]
N_PREFIX = 8


def prefix_choices(n: int, G: int):
    """The eight prefix lengths a row of n keys cycles through: causal, none (pg_attention_rows), one answer token,
    the 64-key block edge and its neighbours, a boundary inside a 16-row wave tile (16 / G positions), and an answer
    that crosses a 64-key block.  Clamped to [1, n]."""
    per = max(16 // G, 1)
    mid = n // 2
    if per > 1 and mid % per == 0:
        mid += 1
    cross = 64 * ((n - 1) // 64) - 3 if n > 64 else n - 3
    out = [1, n, n - 1, 63, 64, 65, mid, cross]
    return [min(max(v, 1), n) for v in out]


def vis(n: int, prefix: int, p: int) -> int:
    return min(n, max(prefix, p + 1))


def _attn_ref_prefix(q, k, v, scale, n, prefix):
    """fp32 softmax attention of one batch row over exactly vis(p) keys per query: q [nh][n][hd], k / v [nh][n][hd]."""
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    p = torch.arange(n, device=s.device)
    seen = torch.minimum(torch.full_like(p, n), torch.clamp(p + 1, min=prefix))
    s = s.masked_fill(torch.arange(n, device=s.device)[None, :] >= seen[:, None], float("-inf"))
    return torch.softmax(s, -1) @ v.float()


def fa_form(B, L, nh, nkv, hd):
    """(query rows per workgroup, keys per block) of the flash form attn_form (csrc/attn.hip) picks for an unmasked
    prefill (its wgs / rounds rules restated)."""
    G, DP = nh // nkv, (hd + 31) // 32 * 32
    wgs = lambda rows: -(-L * G // rows) * nkv * B       # noqa: E731
    rounds = lambda rows: -(-wgs(rows) // 256)           # noqa: E731
    if DP == 256 and wgs(256) >= 256 and rounds(256) * 25 < rounds(128) * 16 and rounds(256) * 25 < rounds(192) * 24:
        return 256, 32
    waves = 8 if wgs(128) >= 256 else 4
    if DP == 256 and waves == 8 and rounds(192) * 12 < rounds(128) * 8:
        waves = 12
    return 16 * waves, 64


def blind_rows(B, L, nh, nkv, hd, nks, lens, pre):
    """Query rows (position < len_b, counted per key split) that sit in a key split which walks at least one block but
    holds no key they see: attn_fa_kernel's walk restated -- a workgroup walks ceil(vis(p_hi) / KB) blocks, dealt
    ceil(blocks / nks) per split.  Such a row's running max is still -inf when the split ends."""
    G = nh // nkv
    rows, KB = fa_form(B, L, nh, nkv, hd)
    R = L * G
    count = 0
    for n, pb in zip(lens, pre):
        for r0 in range(0, R, rows):
            nblk_all = -(-vis(n, pb, min(r0 + rows - 1, R - 1) // G) // KB)
            per = -(-nblk_all // nks)
            for ks in range(nks):
                if min(nblk_all - ks * per, per) <= 0:
                    continue                                     # no block at all: the initial partial, nothing computed
                kb0 = ks * per * KB
                ps = {r // G for r in range(r0, min(r0 + rows, R)) if r // G < n}
                count += G * sum(1 for p in ps if vis(n, pb, p) <= kb0)
    return count


def _kw(B, L, nh, nkv, hd, nks, fallback):
    from pghip import ops
    kw = dict(B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd, scale=hd ** -0.5)
    if nks:
        no, nml = ops.prefill_split_workspace(B, L, nh, nkv, hd, nks)
        kw.update(nsplit=nks, part_o=torch.full((no,), float("nan"), device="cuda"),
                  part_ml=torch.full((nml,), float("nan"), device="cuda"))
    if fallback:    # an all-zero additive mask: the non-flash kernels (attn_kernel, or the LDS kernel from 1024 groups)
        kw.update(mask=torch.zeros(B, L, L, device="cuda"), mask_bs=L * L, mask_rs=L)
    return kw


def _prefix_case(B, L, nh, nkv, hd, nks, fallback, seed=300):
    from pghip import ops
    lens = ragged_lens(B, L)
    Smax = max(320, (L + 8 + 63) // 64 * 64)
    kvd, g = nkv * hd, nh // nkv
    q = rnd(B * L, nh * hd, seed=seed)
    k0 = rnd(B, Smax, kvd, seed=seed + 1)                    # every row finite: stale values past each row's length
    vtc = rnd(B, kvd, Smax, seed=seed + 2)
    qv = q.view(B, L, nh, hd)
    worst, blind = 0.0, 0
    for rnd_i in range(N_PREFIX):
        pre = [prefix_choices(n, g)[(b + rnd_i) % N_PREFIX] for b, n in enumerate(lens)]
        # an off-by-one must show: for every query, keys vis(p) - 1 and vis(p) carry 3x the norm (sharpen's rule) --
        # over a row's queries those are the keys from prefix_b - 1 on, the stale ones past len_b included
        kc = k0.clone()
        for b, pb in enumerate(pre):
            kc[b, pb - 1:] *= 3
        kw = _kw(B, L, nh, nkv, hd, nks, fallback)           # fresh NaN workspaces
        args = (q, nh * hd, None, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax)
        o = torch.full((B * L, nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.attention_prefix(*args[:2], o, *args[3:], lkv_rows=i32(lens), prefix_rows=i32(pre), **kw)
        assert torch.isfinite(o.float()).all(), (rnd_i, "every row must be finite, the padding's included")
        ov = o.view(B, L, nh, hd)
        blind += blind_rows(B, L, nh, nkv, hd, nks, lens, pre) if nks else 0
        for b, (n, pb) in enumerate(zip(lens, pre)):
            kh = kc[b, :n].view(n, nkv, hd).transpose(0, 1).repeat_interleave(g, 0)
            vh = vtc[b, :, :n].view(nkv, hd, n).transpose(1, 2).repeat_interleave(g, 0)
            ref = _attn_ref_prefix(qv[b, :n].transpose(0, 1), kh, vh, hd ** -0.5, n, pb)
            e = err(ov[b, :n].transpose(0, 1), ref)
            worst = max(worst, e)
            assert e < KTOL, (rnd_i, b, n, pb, e)
    print(f"prefix-LM B={B} L={L} hd={hd} nks={nks} fallback={fallback}: worst scaled error {worst:.4f}, "
          f"{blind} rows in a walked split they cannot see into")
    # prefix_b == len_b: pg_attention_rows, bit for bit
    kc = k0.clone()
    args = (q, nh * hd, None, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax)
    a = torch.empty(B * L, nh * hd, dtype=torch.bfloat16, device="cuda")
    b2 = torch.empty_like(a)
    ops.attention_rows(*args[:2], a, *args[3:], lkv_rows=i32(lens), **_kw(B, L, nh, nkv, hd, nks, fallback))
    ops.attention_prefix(*args[:2], b2, *args[3:], lkv_rows=i32(lens), prefix_rows=i32(lens),
                         **_kw(B, L, nh, nkv, hd, nks, fallback))
    assert torch.equal(a, b2)
    # ... and a prefix beyond the row's length is clamped to it
    ops.attention_prefix(*args[:2], b2, *args[3:], lkv_rows=i32(lens), prefix_rows=i32([L + 7] * B),
                         **_kw(B, L, nh, nkv, hd, nks, fallback))
    assert torch.equal(a, b2)
    return blind


def _ids(shapes):
    return ["x".join(str(int(x)) for x in s) for s in shapes]


@pytest.mark.parametrize("shape", SMALL, ids=_ids(SMALL))
def test_prefix_attention_small_shapes(shape):
    """pg_attention_prefix at head_dim 32 / 72 / 128 / 256, MQA and GQA, 4- and 8-wave workgroups: every row's prefix
    walks the eight choices of prefix_choices, against fp32 torch softmax over exactly vis_b(p) keys per query."""
    _prefix_case(*shape)


@pytest.mark.parametrize("shape", FLASH, ids=_ids(FLASH))
def test_prefix_attention_flash_forms(shape):
    """The 12-wave form, the pt-448 batch, 8 waves x 32 rows on 32-key blocks, and the key-split form with
    attn_pf_combine_kernel (workspaces start as NaN): with a causal or short prefix a workgroup near the front of the
    answer stops its walk early and leaves the later splits without a block, whose partial is the initial one."""
    _prefix_case(*shape)


@pytest.mark.parametrize("shape", BLIND, ids=_ids(BLIND))
def test_prefix_attention_key_split_rows_without_a_visible_key(shape):
    """Key splits under 128-row workgroups at G = 1: rows sit in splits that walk blocks of which they see no key, so
    their running max is still -inf at the split's end -- exp2(-inf - -inf) without the kernel's guard, a NaN partial
    that the merge would carry into the output.  blind_rows counts them from the kernel's walk; there must be some,
    every output must be finite and within the bound.  (A build without the guard gives non-finite output here.)"""
    assert fa_form(*shape[:5])[0] == 128
    assert _prefix_case(*shape) > 0


@pytest.mark.parametrize("shape", FALLBACK, ids=_ids(FALLBACK))
def test_prefix_attention_fallback_kernels(shape):
    """Under an additive mask (all zeros) the one-wave kernel and the LDS-staged kernel take the rule too."""
    _prefix_case(*shape)


CENSUS = [(4, 264, 8, 1, 256, 5, False), (4, 150, 4, 1, 32, 0, False), (3, 150, 4, 2, 72, 0, True)]


@pytest.mark.parametrize("shape", CENSUS, ids=_ids(CENSUS))
def test_prefix_attention_census(shape):
    """attn_ref's census (q = 0, one-hot v: every weight exactly 1): query p's output is count_d / vis_b(p) exactly, so
    one key too many or too few anywhere along the causal edge changes a count by one.  Key-split, plain flash and
    one-wave forms."""
    from pghip import ops
    B, L, nh, nkv, hd, nks, fallback = shape
    g = nh // nkv
    lens = ragged_lens(B, L)
    Smax = max(320, (L + 8 + 63) // 64 * 64)
    kvd = nkv * hd
    q, k, v = A.census(B, nh, nkv, L, hd, Smax, lens, seed=21, device="cuda")
    qf, kc, vtc = _layout(q, k, v)
    for rnd_i in range(N_PREFIX):
        pre = [prefix_choices(n, g)[(b + rnd_i) % N_PREFIX] for b, n in enumerate(lens)]
        o = torch.full((B * L, nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.attention_prefix(qf, nh * hd, o, nh * hd, kc, Smax * kvd, hd, kvd, vtc, kvd * Smax, hd * Smax, Smax,
                             lkv_rows=i32(lens), prefix_rows=i32(pre), **_kw(B, L, nh, nkv, hd, nks, fallback))
        assert torch.isfinite(o.float()).all()
        oh = _heads(o, B, L, nh, hd).double().cpu()                      # [B][nh][L][D]
        for b, (n, pb) in enumerate(zip(lens, pre)):
            want = torch.stack([A.census_expected(hd, vis(n, pb, p)) for p in range(n)])      # [n][D]
            bad = (oh[b, :, :n] - want[None]).abs() > A.CENSUS_RTOL * want[None]
            assert not bool(bad.any()), (rnd_i, b, n, pb, bad.nonzero()[0].tolist())


# --------------------------------------------------------------------------------------------- 2. token_logprob
def _lp_ref(x: np.ndarray, targets):
    """float64 numpy: x[t] - logsumexp(x), -inf for a target out of range or a row of nothing but -inf."""
    out = []
    for row, t in zip(np.asarray(x, np.float64), targets):
        m = row.max()
        if not 0 <= t < row.shape[0] or m == -np.inf:
            out.append(-np.inf)
            continue
        out.append(row[t] - (m + np.log(np.exp(row - m).sum())))
    return np.array(out)


@pytest.mark.parametrize("Rr,V,ld", [(1, 1, 1), (3, 300, 304), (5, 257216, 257216), (2, 257217, 257224)])
def test_token_logprob(Rr, V, ld):
    """pg_token_logprob against float64 numpy within PROBS_RTOL of max(1, |ref|): targets at column 0 and V - 1, rows
    with -inf entries (the target's own among them), a row scaled to +-1e4, a row of nothing but -inf, targets out of
    range (-inf, nothing read), and top1 == argmax with the lowest index on a tie.  ld = 1 and V % 4 = 1 take the
    scalar loads."""
    from pghip import ops
    g = torch.Generator().manual_seed(1000 + V)
    base = torch.randn(Rr, ld, generator=g) * 3
    tg = torch.randint(0, V, (Rr,), generator=g)
    tg[0] = 0
    tg[-1] = V - 1 if Rr > 1 else 0
    variants = {}
    variants["plain"] = (base.clone(), tg.clone())
    last = base.clone(); t2 = tg.clone(); t2[0] = V - 1
    variants["last_column"] = (last, t2)
    x = base.clone()
    x[:, :V][torch.rand(Rr, V, generator=g) < 0.3] = float("-inf")
    x[0, tg[0]] = float("-inf")                                  # the target itself: log-prob -inf (or an all -inf row)
    variants["neg_inf"] = (x, tg.clone())
    x = base.clone()
    x[0, :V] = float("-inf")
    variants["all_neg_inf"] = (x, tg.clone())
    x = base.clone()
    x[-1] *= 1e4 / x[-1, :V].abs().max()
    variants["scaled_1e4"] = (x, tg.clone())
    t2 = tg.clone(); t2[0] = V; t2[-1] = -1 if Rr > 1 else V
    variants["out_of_range"] = (base.clone(), t2)
    x = base.clone()
    if V > 1:
        for r in range(Rr):                                      # the row's max twice: the lower index wins
            lo, hi = sorted(torch.randint(0, V, (2,), generator=g).tolist())
            if lo == hi:
                lo, hi = 0, V - 1
            x[r, lo] = x[r, hi] = x[r, :V].max() + 1.0
    variants["tie"] = (x, tg.clone())
    ws = torch.full((ops.token_logprob_workspace(Rr),), 0xFF, dtype=torch.uint8, device="cuda")   # NaN patterns
    for name, (x, t) in variants.items():
        xd = x.cuda()
        lp = torch.full((Rr,), float("nan"), device="cuda")
        top = torch.full((Rr,), -7, dtype=torch.int64, device="cuda")
        ops.token_logprob(xd, t.cuda(), lp, top, ws, V=V)
        ops.token_logprob(xd, t.cuda(), lp2 := torch.full((Rr,), float("nan"), device="cuda"), None, None, V=V)
        got, ref = lp.cpu().numpy().astype(np.float64), _lp_ref(x[:, :V].numpy(), t.tolist())
        assert torch.equal(lp, lp2), name                        # top1 is optional
        assert not np.isnan(got).any(), (name, got)
        inf = np.isinf(ref)
        assert (got[inf] == ref[inf]).all(), (name, got, ref)
        rel = np.abs(got[~inf] - ref[~inf]) / np.maximum(1.0, np.abs(ref[~inf]))
        print(f"token_logprob R={Rr} V={V} {name}: worst {rel.max() if rel.size else 0.0:.2e}")
        assert (rel <= PROBS_RTOL).all(), (name, got, ref)
        want = np.argmax(x[:, :V].numpy(), -1)                   # (numpy: the first index of the maximum)
        assert top.cpu().tolist() == want.tolist(), (name, top, want)
        assert top.cpu().tolist() == torch.argmax(x[:, :V], -1).tolist(), name
        if name == "out_of_range":
            assert np.isinf(got[0]) and got[0] < 0 and np.isinf(got[-1])


# ------------------------------------------------------------------------------------------------------ 3. engine
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


def _score(eng, answers, **kw):
    ids, mask, types, px, prefix = S.batch(answers)
    t = lambda a: torch.from_numpy(a).cuda()             # noqa: E731
    out = eng.score(t(ids), t(px), t(mask), t(types), **kw)
    torch.cuda.synchronize()
    return out


def _check_against(out, answers, refs, tol, margin_floor=0.0):
    """The rows of a score() result against per-row oracle logits: logits within `tol` (scaled max error), log-probs
    within 2 tol max|ref logits| nats of the reference's log-softmax, top1 the oracle's argmax where its margin exceeds
    ragged_ref.MARGIN (and margin_floor).  Returns how many steps exceeded the margin."""
    B = len(answers)
    S_max = max(len(a) for a in answers)
    lp, t1, lg = out["logprobs"].cpu().numpy(), out["top1"].cpu().numpy(), out["logits"].cpu().numpy()
    assert out["suffix_lens"].tolist() == [len(a) for a in answers]
    assert lp.shape == (B, S_max) and t1.shape == (B, S_max) and lg.shape[0] == sum(len(a) for a in answers)
    off, decided, worst, worst_lp = 0, 0, 0.0, 0.0
    for b, a in enumerate(answers):
        for t, tok in enumerate(a):
            ref = np.asarray(refs[b][t], np.float64)[0]
            e = nerr(lg[off + t][None], ref[None])
            worst = max(worst, e)
            assert e < tol, (b, t, e)
            want = S.log_softmax64(ref)[int(tok)]
            d = abs(float(lp[b, t]) - want)
            worst_lp = max(worst_lp, d)
            assert d <= 2 * tol * np.abs(ref).max(), (b, t, float(lp[b, t]), want)
            top = np.sort(ref)[::-1]
            if top[0] - top[1] > max(R.MARGIN, margin_floor):
                decided += 1
                assert int(t1[b, t]) == int(np.argmax(ref)), (b, t)
        assert (lp[b, len(a):] == 0).all() and (t1[b, len(a):] == R.PAD).all(), b
        off += len(a)
    print(f"score: worst scaled logit error {worst:.4f}, worst log-prob error {worst_lp:.4f} nats, "
          f"{decided} steps above the margin")
    return decided


def test_score_greedy_answers_vs_oracle(tiny):
    """The first 8 pool requests, each followed by the oracle's own 16 greedy tokens: score()'s logits rows against the
    oracle's per-step logits, log-probs against their log-softmax, top1 against the oracle's ids.  Measured on the
    CPU, 94 of the 128 steps have a margin above 0.1; at least 64 must."""
    refs = [R.reference(b) for b in range(8)]
    answers = [list(r[0]) for r in refs]
    out = _score(tiny, answers, return_logits=True)
    decided = _check_against(out, answers, [r[1] for r in refs], TOL)
    assert decided >= 64, decided
    for b, r in enumerate(refs):                         # (the oracle's greedy ids are its argmax: the same thing)
        for t in range(R.STEPS):
            if r[2][t] > R.MARGIN:
                assert int(out["top1"][b, t]) == r[0][t], (b, t)
    plain = _score(tiny, answers)
    assert set(plain) == {"logprobs", "top1", "suffix_lens"}
    assert torch.equal(plain["logprobs"], out["logprobs"]) and torch.equal(plain["top1"], out["top1"])


def test_score_arbitrary_answers_vs_oracle(tiny):
    """Seeded random answers of lengths 16, 1, 7, 2, 16, 3, 9, 5 (rows differ in prefix and in answer length) against
    the oracle fed one answer token at a time through its KVCache (score_ref); the same bounds."""
    refs = [S.reference(b) for b in range(8)]
    answers = [list(r[0]) for r in refs]
    out = _score(tiny, answers, return_logits=True)
    _check_against(out, answers, [r[1] for r in refs], TOL)


def test_score_is_causal(tiny):
    """Two calls that differ only in each row's last answer token: no row that is used sees that token, so every
    logits row is bit-identical (and every log-prob but each row's last)."""
    answers = [list(S.reference(b)[0]) for b in range(8)]
    other = [a[:-1] + [3 + (a[-1] - 3 + 17) % 296] for a in answers]
    assert all(a[-1] != o[-1] and 3 <= o[-1] < 299 for a, o in zip(answers, other))
    x, y = _score(tiny, answers, return_logits=True), _score(tiny, other, return_logits=True)
    assert torch.equal(x["logits"], y["logits"])
    assert torch.equal(x["top1"], y["top1"])
    for b, a in enumerate(answers):
        assert torch.equal(x["logprobs"][b, :len(a) - 1], y["logprobs"][b, :len(a) - 1])
        assert float(x["logprobs"][b, len(a) - 1]) != float(y["logprobs"][b, len(a) - 1])


def test_score_chunking_keeps_the_bits(tiny):
    """SCORE_CHUNK_ROWS = 5 (12 lm_head launches over the 59 answer rows, the last of 4 rows) against the default 128
    (one launch): the same logits, log-probs and top1, bit for bit."""
    answers = [list(S.reference(b)[0]) for b in range(8)]
    whole = _score(tiny, answers, return_logits=True)
    tiny.SCORE_CHUNK_ROWS = 5
    try:
        parts = _score(tiny, answers, return_logits=True)
    finally:
        tiny.SCORE_CHUNK_ROWS = type(tiny).SCORE_CHUNK_ROWS
    assert type(tiny).SCORE_CHUNK_ROWS == 128
    for k in ("logits", "logprobs", "top1"):
        assert torch.equal(whole[k], parts[k]), k


def test_score_fp8_vs_oracle(tiny_fp8):
    """fp8 engine (the prefill's B * L rows are far above 16: every Gemma linear on e4m3 operands; score()'s lm_head
    stays on the bf16 weights).  Bound by the rule of test_ragged_fp8_batch_17_vs_oracle: 1.5x the distance of the
    oracle run on the same operand rounding (bf16_operands + fp8_operands(min_rows=0)) from the fp32 oracle, computed
    here per row and step, the largest taken."""
    from oracle import paligemma_oracle as O
    B = 4
    refs = [R.reference(b) for b in range(B)]
    answers = [list(r[0]) for r in refs]
    ie = []
    for b in range(B):
        with O.bf16_operands(), O.fp8_operands(min_rows=0, lm_head=False):
            emu = S.teacher_forced(b, answers[b])
        ie += [nerr(emu[t], refs[b][1][t]) for t in range(len(answers[b]))]
    bound = 1.5 * max(ie)
    amax = max(float(np.abs(lg).max()) for r in refs for lg in r[1])
    out = _score(tiny_fp8, answers, return_logits=True)
    _check_against(out, answers, [r[1] for r in refs], bound, margin_floor=2 * bound * amax)
    print(f"score fp8: bound {bound:.4f} (emulated oracle {max(ie):.4f})")


def test_model_score_returns_the_engines_result():
    from oracle import configs as ocfg, synth
    from modeling_paligemma import PaliGemmaConfig, PaliGemmaForConditionalGeneration
    m = PaliGemmaForConditionalGeneration(PaliGemmaConfig(**ocfg.TINY))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.generate_state_dict(ocfg.TINY).items()}, strict=False)
    m.tie_weights()
    m = m.to("cuda").eval()
    answers = [list(S.reference(b)[0]) for b in range(3)]
    ids, mask, types, px, _ = S.batch(answers)
    t = lambda a: torch.from_numpy(a).cuda()             # noqa: E731
    got = m.score(t(ids), t(px), t(mask), t(types), return_logits=True)
    want = m.engine(t(ids).device).score(t(ids), t(px), t(mask), t(types), return_logits=True)
    assert set(got) == {"logprobs", "top1", "suffix_lens", "logits"}
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert not got["logprobs"].requires_grad
    _check_against(got, answers, [S.reference(b)[1] for b in range(3)], TOL)
