"""Beam search on the device: pg_beam_select, pg_kv_beam_gather and PaliGemmaEngine.generate_beam.

References live in tests/beam_ref.py (float64 numpy, no GPU code).  Bounds are the project's existing ones: a float32
log-probability against float64 within PROBS_RTOL of max(1, |ref|) (test_attn_structured_gpu.PROBS_RTOL, the bound
test_score_gpu.test_token_logprob holds the same log-sum-exp to); logits against the oracle within TOL = 3e-2, so a
summed log-probability within 2 * TOL * max |reference logit| per generated token (test_score_gpu's rule); hypotheses
and their order equal the oracle's where its candidates are more than ragged_ref.MARGIN apart (beam_ref.REQUESTS).
Everything else here is exact: ties, frozen beams, the KV reorder byte for byte, graph replay against eager, and the
beam run's logits against a teacher-forced run of the same hypotheses."""
import numpy as np
import pytest
import torch

import beam_ref as BR
import ragged_ref as R
from test_attn_structured_gpu import PROBS_RTOL
from test_ragged_gpu import TOL

pytestmark = pytest.mark.gpu

PAD, STOP = 0, 1
NEW = 12             # engine tests: prompt 0 (19 keys) crosses key 32 mid-run


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------------ helpers
GUARD = 16


class Guarded:
    """A device tensor of n elements between two guard runs of a sentinel, in one allocation."""

    def __init__(self, init, sentinel):
        init = torch.as_tensor(init)
        self.n = init.numel()
        self.buf = torch.full((self.n + 2 * GUARD,), sentinel, dtype=init.dtype, device="cuda")
        self.sentinel = sentinel
        self.t = self.buf[GUARD:GUARD + self.n]
        self.t.copy_(init.reshape(-1))

    def intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]).cpu()
        if g.dtype.is_floating_point and self.sentinel != self.sentinel:
            return bool(torch.isnan(g).all())
        return bool((g == self.sentinel).all())


def _logits_dev(x, V, ld):
    """x [rows][V] inside NaN-poisoned padding columns and a NaN-poisoned allocation; the view [rows][V], stride ld."""
    rows = x.shape[0]
    flat = torch.full((8 + rows * ld,), float("nan"), dtype=torch.float32)
    body = flat[4:4 + rows * ld].view(rows, ld)
    body[:, :V] = x
    dev = flat.cuda()
    return dev, dev[4:4 + rows * ld].view(rows, ld)[:, :V]


def run_select(x, V, ld, W, cum, fin, stop, pad=PAD, hist_rows=4, step0=1, advance=True):
    """One ops.beam_select call on guarded buffers; returns a dict of host copies after checking every guard."""
    from pghip import ops
    rows = x.shape[0]
    _, xd = _logits_dev(x, V, ld)
    g = dict(cum=Guarded(torch.as_tensor(cum, dtype=torch.float32), float("nan")),
             fin=Guarded(torch.as_tensor(fin, dtype=torch.int32), -77),
             ids=Guarded(torch.full((rows,), -5, dtype=torch.int64), -99),
             par=Guarded(torch.full((rows,), -5, dtype=torch.int32), -99),
             ht=Guarded(torch.full((hist_rows * rows,), -3, dtype=torch.int64), -99),
             hp=Guarded(torch.full((hist_rows * rows,), -3, dtype=torch.int32), -99),
             step=Guarded(torch.tensor([step0], dtype=torch.int32), -99),
             pos=Guarded(torch.arange(100, 100 + rows, dtype=torch.int32), -99),
             kv=Guarded(torch.tensor([40], dtype=torch.int32), -99),
             flag=Guarded(torch.tensor([-1], dtype=torch.int32), -99),
             ws=Guarded(torch.zeros(ops.beam_select_workspace(rows, W) + 16, dtype=torch.uint8), 0xA5))
    off = (-g["ws"].t.data_ptr()) % 16                         # the workspace must be 16-B aligned
    ws = g["ws"].t[off:off + ops.beam_select_workspace(rows, W)]
    ops.beam_select(xd, g["cum"].t, g["fin"].t, g["ids"].t, g["par"].t, ws, W=W, stop_token=stop, pad_token=pad,
                    hist_tok=g["ht"].t.view(hist_rows, rows), hist_parent=g["hp"].t.view(hist_rows, rows),
                    step=g["step"].t, pos=g["pos"].t if advance else None, kv_len=g["kv"].t if advance else None,
                    flag=g["flag"].t)
    torch.cuda.synchronize()
    for k, v in g.items():
        assert v.intact(), f"guard words around {k} were written"
    out = {k: v.t.cpu().clone() for k, v in g.items() if k != "ws"}
    out["ht"], out["hp"] = out["ht"].view(hist_rows, rows), out["hp"].view(hist_rows, rows)
    # the decode-state advance pg_argmax does
    assert int(out["step"]) == step0 + 1
    if step0 < hist_rows:
        assert out["ht"][step0].tolist() == out["ids"].tolist() and out["hp"][step0].tolist() == out["par"].tolist()
        untouched = [s for s in range(hist_rows) if s != step0]
    else:
        untouched = list(range(hist_rows))
    assert bool((out["ht"][untouched] == -3).all()) and bool((out["hp"][untouched] == -3).all())
    assert out["pos"].tolist() == [100 + r + int(advance) for r in range(rows)]
    assert int(out["kv"]) == 40 + int(advance)
    assert int(out["flag"]) == int(bool((out["fin"] != 0).all()))
    return out


def _check(x, W, cum, fin, stop, out, pad=PAD):
    BR.check_select(x.numpy(), np.asarray(cum, np.float64), np.asarray(fin), W, stop, pad, out["ids"].numpy(),
                    out["par"].numpy(), out["cum"].numpy().astype(np.float64), out["fin"].numpy(), PROBS_RTOL)


# ------------------------------------------------------------------------------------------------ 1. selection
SELECT_CASES = [(V, ld, W, B) for V, ld in ((17, 20), (300, 304), (300, 301), (4100, 4112)) for W in (1, 2, 3, 8)
                for B in (1, 3)] + [(257216, 257216, W, B) for W, B in ((1, 1), (2, 3), (3, 3), (8, 1))]


@pytest.mark.parametrize("V,ld,W,B", SELECT_CASES)
def test_beam_select_against_float64(V, ld, W, B):
    """pg_beam_select against beam_ref.select's rules on the same fp32 logits: V = 17 (fewer columns than a row has
    workgroups), 300 (ld 304: aligned rows; ld 301: odd rows misaligned, scalar loads), 4100 of 4112 (a ragged last
    vector, every row 16-B aligned), 257216 (four vectors per thread; at four (W, B) pairs).  Random scores, the first step
    (cum = 0, -inf, ...: the row's top W ids in order, exactly), some beams finished, a stop token among the winners,
    and two consecutive calls giving identical bits."""
    g = torch.Generator().manual_seed(7 * V + 31 * W + B)
    rows = B * W
    x = torch.randn(rows, V, generator=g) * 3
    # random scores
    cum = -torch.rand(rows, generator=g) * 20
    fin = torch.zeros(rows, dtype=torch.int32)
    out = run_select(x, V, ld, W, cum, fin, None)
    _check(x, W, cum, fin, None, out)
    again = run_select(x, V, ld, W, cum, fin, None)
    for k in ("ids", "par", "cum", "fin", "ht", "hp", "flag"):
        assert torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), k
    # the winner of group 0 as the stop token: that row finishes, and only rows that took it
    stop = int(out["ids"][0])
    o2 = run_select(x, V, ld, W, cum, fin, stop)
    _check(x, W, cum, fin, stop, o2)
    assert o2["ids"].tolist() == out["ids"].tolist() and int(o2["fin"][0]) == 1
    assert o2["fin"].tolist() == [int(t == stop) for t in out["ids"].tolist()]
    # the first step: only beam 0 of a group can win, its top W ids in order (no tolerance: one row, ordered by logit)
    cum0 = torch.full((rows,), float("-inf"))
    cum0[::W] = 0.0
    o3 = run_select(x, V, ld, W, cum0, fin, None, step0=0, advance=False)
    for b in range(B):
        order = np.lexsort((np.arange(V), -x[b * W].numpy().astype(np.float64)))[:W]
        assert o3["ids"][b * W:(b + 1) * W].tolist() == order.tolist(), b
        assert o3["par"][b * W:(b + 1) * W].tolist() == [b * W] * W
    _check(x, W, cum0, fin, None, o3)
    # some beams finished (every group keeps at least its frozen candidates in play)
    if W > 1:
        fin2 = (torch.rand(rows, generator=g) < 0.5).to(torch.int32)
        fin2[0] = 1
        o4 = run_select(x, V, ld, W, cum, fin2, None)
        _check(x, W, cum, fin2, None, o4)


def _spaced(rows, V, seed, gap=0.5):
    """Logits whose values within a row are a permutation of gap * (0 .. V - 1): every pair at least `gap` apart."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(V, generator=g).float() * gap - gap * V / 2 for _ in range(rows)])


def test_beam_select_exact_ties_and_frozen_beams():
    """The cases that take no tolerance, V = 300 (ld 304), W = 3, B = 2."""
    V, ld, W, B = 300, 304, 3, 2
    rows = B * W
    zero = torch.zeros(rows, dtype=torch.int32)
    # two parents with bit-identical logits and equal cum: the lower parent first, candidate by candidate
    x = _spaced(rows, V, 1)
    x[1] = x[0]
    cum = torch.tensor([-1.0, -1.0, -50.0, -2.0, -3.0, -4.0])
    out = run_select(x, V, ld, W, cum, zero, None)
    ids, par, _, _, _ = BR.select(x.numpy(), cum.numpy(), zero.numpy(), W, None, PAD)
    best = int(torch.argmax(x[0]))
    assert out["par"][:3].tolist() == [0, 1, 0] and out["ids"][:2].tolist() == [best, best]
    assert out["ids"].tolist() == ids.tolist() and out["par"].tolist() == par.tolist()
    assert out["cum"][0].item() == out["cum"][1].item()
    # equal logits at two ids: the lower id wins, at every rank it can (the maximum twice, then the runner-up twice)
    x = _spaced(rows, V, 2)
    top = x[0].max().item()
    x[0, 200] = x[0, 7] = top + 1.0
    x[0, 150] = x[0, 40] = top + 0.25
    cum0 = torch.tensor([0.0, float("-inf"), float("-inf"), 0.0, float("-inf"), float("-inf")])
    out = run_select(x, V, ld, W, cum0, zero, None, step0=0, advance=False)
    assert out["ids"][:3].tolist() == [7, 200, 40] and out["par"][:3].tolist() == [0, 0, 0]
    assert out["cum"][0].item() == out["cum"][1].item()
    # a finished parent yields exactly (parent, pad, the same cum), wherever its score ranks
    x = _spaced(rows, V, 3)
    cum = torch.tensor([-30.0, -0.125, -31.0, -2.0, -90.0, -3.0])
    fin = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.int32)
    out = run_select(x, V, ld, W, cum, fin, STOP)
    assert (out["ids"][0].item(), out["par"][0].item(), out["cum"][0].item(), out["fin"][0].item()) == (PAD, 1, -0.125, 1)
    assert 4 not in out["par"].tolist()                     # -90 loses to live candidates: a frozen beam can drop out
    assert out["par"].tolist().count(1) == 1                # ... and is offered once, not V times
    _check(x, W, cum, fin, STOP, out)
    assert int(out["flag"]) == 0
    # all beams finished: the flag is set, every id is pad, the scores are unchanged (sorted, ties to the lower beam)
    cum = torch.tensor([-3.0, -1.0, -3.0, -0.5, -0.5, -7.0])
    fin = torch.ones(rows, dtype=torch.int32)
    out = run_select(x, V, ld, W, cum, fin, STOP)
    assert int(out["flag"]) == 1 and out["ids"].tolist() == [PAD] * rows and out["fin"].tolist() == [1] * rows
    assert out["par"].tolist() == [1, 0, 2, 3, 4, 5] and out["cum"].tolist() == [-1.0, -3.0, -3.0, -0.5, -0.5, -7.0]
    # the stop token taken: finished is set for that row only
    x = _spaced(rows, V, 4)
    x[0, STOP] = x[0].max() + 5.0
    cum = torch.tensor([-1.0, -1.5, -2.0, -1.0, -1.5, -2.0])
    out = run_select(x, V, ld, W, cum, zero, STOP)
    assert out["ids"][0].item() == STOP and out["par"][0].item() == 0
    assert out["fin"].tolist() == [int(t == STOP) for t in out["ids"].tolist()] and out["fin"].tolist().count(1) == 1
    assert int(out["flag"]) == 0
    # with *step == hist_rows nothing is written past (or into) the histories: run_select checks them and the guards
    run_select(x, V, ld, W, cum, zero, STOP, hist_rows=2, step0=2)
    run_select(x, V, ld, W, cum, zero, STOP, hist_rows=2, step0=1)


@pytest.mark.parametrize("V,ld", [(300, 304), (4100, 4112)])
def test_beam_select_nan_and_inf_rows(V, ld):
    """Rows of -inf and a row with NaNs: no NaN wins while a comparable candidate is left, no id falls outside [0, V),
    no parent outside its group -- also when nothing comparable is left at all."""
    W, B = 3, 2
    rows = B * W
    g = torch.Generator().manual_seed(V)
    zero = torch.zeros(rows, dtype=torch.int32)
    cum = -torch.rand(rows, generator=g)
    x = torch.randn(rows, V, generator=g)
    x[0] = float("-inf")                                    # a row of nothing but -inf: its candidates score -inf
    x[1, 5] = float("nan")                                  # a row with a NaN: its log-sum-exp, so its scores, are NaN
    x[4, ::7] = float("-inf")                               # -inf entries are legal and add nothing
    out = run_select(x, V, ld, W, cum, zero, None)
    assert out["par"][:3].tolist() == [2, 2, 2] and not torch.isnan(out["cum"]).any()
    _check(x, W, cum, zero, None, out)
    x[2] = float("-inf")                                    # group 0: -inf, NaN, -inf -- the -inf candidates beat the NaN
    out = run_select(x, V, ld, W, cum, zero, None)
    assert set(out["par"][:3].tolist()) <= {0, 2} and bool((out["cum"][:3] == float("-inf")).all())
    assert out["par"][:3].tolist() == [0, 0, 0] and out["ids"][:3].tolist() == [0, 1, 2]      # ties: the lowest (p, t)
    x[:] = float("nan")                                     # nothing comparable anywhere
    out = run_select(x, V, ld, W, cum, zero, None)
    assert bool(((out["ids"] >= 0) & (out["ids"] < V)).all())
    assert all(b * W <= p < (b + 1) * W for b in range(B) for p in out["par"][b * W:(b + 1) * W].tolist())
    # a frozen beam is comparable: it beats a group of NaN rows
    fin = torch.tensor([0, 0, 1, 0, 0, 0], dtype=torch.int32)
    out = run_select(x, V, ld, W, cum, fin, None)
    assert (out["ids"][0].item(), out["par"][0].item(), out["cum"][0].item()) == (PAD, 2, cum[2].item())


def test_beam_select_rejects_bad_shapes():
    from pghip import ops
    x = torch.zeros(18, 300, device="cuda")
    mk = lambda n: (torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),  # noqa: E731
                    torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.beam_select(x, *mk(18), W=9)
    with pytest.raises(ValueError):
        ops.beam_select(x, *mk(18), W=4)                     # rows not a multiple of W
    with pytest.raises(ValueError):
        ops.beam_select(x[:4, :3], *mk(4), W=4)              # W > V
    with pytest.raises(ValueError):
        ops.beam_select(x, *mk(18), W=3, pad_token=300)
    with pytest.raises(TypeError):
        ops.beam_select(x.double(), *mk(18), W=3)
    with pytest.raises(ValueError):
        ops.beam_select_workspace(18, 0)


# ------------------------------------------------------------------------------------------------ 2. KV reorder
PAIRS = [(19, 20), (19, 33), (31, 32), (32, 33), (64, 96), (65, 97), (5, 70)]
SMAX, LAYERS = 128, 2


def _parent_maps(rows):
    if rows == 2:
        return {"identity": [0, 1], "swap": [1, 0], "all_from_last": [1, 1]}
    if rows == 3:
        return {"identity": [0, 1, 2], "swap": [1, 0, 2], "cycle": [1, 2, 0], "all_from_last": [2, 2, 2]}
    return {"identity": list(range(8)), "swap": [1, 0, 2, 3, 4, 5, 7, 6], "cycle": [1, 2, 0, 3, 4, 6, 7, 5],
            "all_from_last": [3, 3, 3, 3, 7, 7, 7, 7], "mixed": [1, 0, 3, 3, 4, 4, 6, 5]}


def _canon(kd, vd, Hkv, D):
    """Decode-order arrays [layers][rows][Hkv][Smax * D] back to [layers][rows][Smax][Hkv * D] by beam_ref's maps."""
    ko, vo = BR.dec_maps(SMAX, D)
    k = np.concatenate([kd[:, :, h][:, :, ko] for h in range(Hkv)], axis=-1)
    v = np.concatenate([vd[:, :, h][:, :, vo] for h in range(Hkv)], axis=-1)
    return k, v


@pytest.mark.parametrize("Hkv,D", [(1, 32), (1, 256), (2, 32)])
@pytest.mark.parametrize("rows", [2, 3, 8])
def test_kv_beam_gather(Hkv, D, rows):
    """pg_kv_beam_gather against beam_ref.gather in all four layouts, byte for byte: TINY's geometry, the real one
    (Hkv 1, D 256) and two kv heads; 2 layers, Smax 128; groups with a common random prompt and distinct suffixes (and
    distinct dead slots past the length); every parent map and (base, len) pair, in the per-row and the shared length
    form.  Positions [base, len) must be the parent's, [floor32(base), base) and everything outside the 32-key window
    must keep their bytes, dead slots inside the window may be the row's own or the parent's."""
    from pghip import ops
    kvd = Hkv * D
    W = 4 if rows == 8 else rows
    rng = np.random.default_rng([Hkv, D, rows])
    S_scr = 128
    scratch = torch.full((ops.kv_beam_gather_scratch(LAYERS, rows, S_scr, kvd),), float("nan"), dtype=torch.bfloat16,
                         device="cuda")
    for pi, (base, length) in enumerate(PAIRS):
        k = rng.integers(-32768, 32767, size=(LAYERS, rows, SMAX, kvd), dtype=np.int16)
        v = rng.integers(-32768, 32767, size=(LAYERS, rows, SMAX, kvd), dtype=np.int16)
        for g in range(rows // W):                          # the group's common prompt
            k[:, g * W:(g + 1) * W, :base] = k[:, g * W:g * W + 1, :base]
            v[:, g * W:(g + 1) * W, :base] = v[:, g * W:g * W + 1, :base]
        vt = np.ascontiguousarray(v.transpose(0, 1, 3, 2))
        kd, vd = BR.pack_dec(k, vt, Hkv)
        if pi == 0:                                         # beam_ref's own maps are the library's
            kd_o, vd_o = ops.decode_cache_pack(torch.from_numpy(k[0]).cuda(), torch.from_numpy(vt[0]).cuda(), Hkv)
            assert np.array_equal(kd_o.cpu().numpy().reshape(kd[0].shape), kd[0])
            assert np.array_equal(vd_o.cpu().numpy().reshape(vd[0].shape), vd[0])
        bases = np.full(rows, base)
        lens = np.full(rows, length)
        for name, parent in _parent_maps(rows).items():
            for per_row in (True, False):
                hold = [Guarded(torch.from_numpy(a), 0x7FC1) for a in (k, vt, kd, vd)]
                t = [h.t.view(torch.bfloat16) for h in hold]
                # the device lengths as the decode step holds them after its sampler: pos = len + 1 per row, or kv_len
                len_dev = torch.tensor((lens + 1).tolist() if per_row else [length], dtype=torch.int32, device="cuda")
                ops.kv_beam_gather(t[0].view(LAYERS, rows, SMAX, kvd), t[1].view(LAYERS, rows, kvd, SMAX),
                                   t[2].view(LAYERS, -1), t[3].view(LAYERS, -1),
                                   torch.tensor(parent, dtype=torch.int32, device="cuda"),
                                   torch.tensor(bases.tolist(), dtype=torch.int32, device="cuda"), len_dev, scratch,
                                   kv_heads=Hkv, len_rows=per_row, len_base=-1 if per_row else 0, S_scr=S_scr)
                torch.cuda.synchronize()
                assert all(h.intact() for h in hold), (name, base, length)
                got = [h.t.cpu().numpy() for h in hold]
                gk = got[0].reshape(k.shape)
                gv = got[1].reshape(vt.shape).transpose(0, 1, 3, 2)
                gkd, gvd = _canon(got[2].reshape(kd.shape), got[3].reshape(vd.shape), Hkv, D)
                wk, wvt, wkd, wvd = BR.gather(k, vt, kd, vd, parent, bases, lens, Hkv)
                wkd_c, wvd_c = _canon(wkd, wvd, Hkv, D)
                lo, hi = base // 32 * 32, -(-length // 32) * 32
                for what, g_, want, old in (("k", gk, wk, k), ("vt", gv, wvt.transpose(0, 1, 3, 2), v),
                                            ("kd", gkd, wkd_c, k), ("vd", gvd, wvd_c, v)):
                    tag = (what, name, base, length, per_row)
                    assert np.array_equal(want[:, :, :length], g_[:, :, :length]), tag      # the contract, and the prompt
                    assert np.array_equal(old[:, :, :lo], g_[:, :, :lo]) and np.array_equal(old[:, :, hi:], g_[:, :, hi:]), tag
                    for r, p in enumerate(parent):
                        dead = g_[:, r, length:hi]
                        if p == r:
                            assert np.array_equal(dead, old[:, r, length:hi]), tag
                        else:
                            assert bool(((dead == old[:, r, length:hi]) | (dead == old[:, p, length:hi])).all()), tag
                    if name == "identity":
                        assert np.array_equal(old, g_), tag


def test_kv_beam_gather_rejects_bad_arguments():
    from pghip import ops
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    i = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")      # noqa: E731
    k, vt, kd, vd = z(2, 2, 64, 32), z(2, 2, 32, 64), z(2, 2 * 64 * 32), z(2, 2 * 64 * 32)
    sc = z(ops.kv_beam_gather_scratch(2, 2, 32, 32))
    kw = dict(kv_heads=1, len_rows=True, len_base=-1, S_scr=32)
    ops.kv_beam_gather(k, vt, kd, vd, i(2), i(2), i(2), sc, **kw)       # legal (nothing to move)
    with pytest.raises(ValueError):
        ops.kv_beam_gather(k, vt, kd, vd, i(2), i(2), i(2), sc[:-1], **kw)
    with pytest.raises(ValueError):
        ops.kv_beam_gather(k, vt, kd, vd, i(3), i(2), i(2), sc, **kw)
    with pytest.raises(ValueError):
        ops.kv_beam_gather(k, vt, kd, vd, i(2), i(2), i(2), sc, **dict(kw, S_scr=40))
    with pytest.raises(TypeError):
        ops.kv_beam_gather(k.float(), vt, kd, vd, i(2), i(2), i(2), sc, **kw)


# ------------------------------------------------------------------------------------------------ 3. engine (TINY)
@pytest.fixture(scope="module")
def tiny():
    from pghip import configs, engine, synthetic, weights
    cfg = configs.TINY
    return engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__))


def _t(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def _pool_batch(reqs):
    """(ids, mask, px) right-padded, of (pool request, seed) pairs."""
    rs = [R.request(b, seed) for b, seed in reqs]
    L = max(r[0].shape[1] for r in rs)
    ids = np.full((len(rs), L), R.PAD, dtype=np.int64)
    mask = np.zeros((len(rs), L), dtype=np.int64)
    for i, (r, _) in enumerate(rs):
        ids[i, :r.shape[1]] = r[0]
        mask[i, :r.shape[1]] = 1
    return ids, mask, np.concatenate([p for _, p in rs])


def _lp64(row, t):
    return float(BR.row_scores(row, 0.0)[t])


def test_one_beam_is_greedy(tiny):
    """generate_beam(num_beams=1) returns exactly generate's greedy ids for a ragged batch of pool rows 0..3, and its
    sum_logprobs are the sums of the traced per-step log-probabilities (within PROBS_RTOL per step)."""
    ids, mask, px, _ = R.batch(4)
    want = tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=None)
    got = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, 1, stop_token=None, return_trace=True)
    assert [s[0] for s in got["sequences"]] == want.tolist()
    assert got["parents"].tolist() == [[0, 1, 2, 3]] * NEW
    for b in range(4):
        s = sum(_lp64(got["logits"][t][b].cpu().numpy(), int(got["tokens"][t][b])) for t in range(NEW))
        assert abs(float(got["sum_logprobs"][b, 0]) - s) <= NEW * PROBS_RTOL * max(1.0, abs(s)), (b, s)
        assert abs(float(got["scores"][b, 0]) - s / NEW) <= PROBS_RTOL * max(1.0, abs(s)), b
    # with the default stop token the sequences end where generate's rows end
    rows = tiny.generate(_t(ids), _t(px), _t(mask), NEW, return_list=True)
    got = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, 1)
    assert [s[0] for s in got["sequences"]] == rows


@pytest.mark.parametrize("B,W,pool", [(1, 2, [0]), (1, 3, [6]), (2, 4, [4, 5]), (3, 8, [0, 4, 5])])
def test_ancestry_teacher_forced(tiny, B, W, pool):
    """Each final hypothesis, teacher-forced in its final row over a fresh replicated cache with no reordering,
    reproduces bit for bit the logits the beam run computed along that hypothesis's ancestry: so every generated key
    and value followed its hypothesis through every reorder, in whichever layout the step's attention reads.  2 rows
    run the fused-finalised route, 3 the unfused one, 8 the 5..16-row route, 24 the route above 16 rows.  The trace's
    selections are re-checked against float64."""
    ids, mask, px, _ = R.batch(B, rows=pool)
    out = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, W, stop_token=None, return_trace=True,
                             num_return_sequences=W)
    rows = B * W
    tok, par = out["tokens"].numpy(), out["parents"].numpy()
    assert tok.shape == (NEW, rows)
    # the selections, step by step
    cum = np.full(rows, -np.inf)
    cum[::W] = 0.0
    zero = np.zeros(rows, np.int64)
    for t in range(NEW):
        lg = out["logits"][t].cpu().numpy()
        BR.check_select(lg, cum, zero, W, None, PAD, tok[t], par[t], out["cum"][t].numpy().astype(np.float64), zero,
                        PROBS_RTOL)
        cum = out["cum"][t].numpy().astype(np.float64)
    # at least one reorder that is not the identity happened, or the test shows nothing about the gather
    assert any(par[t].tolist() != list(range(rows)) for t in range(1, NEW)), "every step kept every row in place"
    hyp = BR.backtrack(tok, par)
    anc = [BR.ancestry(par, r) for r in range(rows)]
    cache0, feats, logits0, nxt = tiny.prefill_request(_t(ids), _t(px), _t(mask), NEW)
    cache = cache0.repeat_rows(W)
    first = logits0[:, :tiny.w.vocab].repeat_interleave(W, dim=0)
    assert torch.equal(out["logits"][0], first)
    st = tiny.decode_state(rows, cache, nxt.repeat_interleave(W), NEW)
    for t in range(1, NEW):
        st["ids"].copy_(torch.tensor([h[t - 1] for h in hyp], dtype=torch.int64))
        lg = tiny.decode_step(st, cache, feats, None)
        want = out["logits"][t][torch.tensor([a[t - 1] for a in anc], device="cuda")]
        bad = (lg != want).any(-1).nonzero().flatten().tolist()
        assert not bad, (t, bad, float((lg - want).abs().max()))
        st["pos"] += 1                                          # the advance a sampler would make
        if not st["ragged"]:
            st["kv_len"] += 1


@pytest.mark.parametrize("B,W,pool", [(1, 3, [6]), (2, 4, [4, 5])])
def test_graph_replay_equals_eager(tiny, B, W, pool):
    ids, mask, px, _ = R.batch(B, rows=pool)
    a = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, W, stop_token=None, return_trace=True,
                           num_return_sequences=W, use_graph=True)
    b = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, W, stop_token=None, return_trace=True,
                           num_return_sequences=W, use_graph=False)
    assert a["sequences"] == b["sequences"]
    for k in ("tokens", "parents", "beam_rows"):
        assert torch.equal(a[k], b[k]), k
    for k in ("cum", "scores", "sum_logprobs"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for x, y in zip(a["logits"], b["logits"]):
        assert torch.equal(x, y)


_ORACLE_RUN = {}


def _oracle_run(tiny):
    """One generate_beam call over beam_ref.REQUESTS (a ragged batch), shared by the oracle tests."""
    if "out" not in _ORACLE_RUN:
        ids, mask, px = _pool_batch([r[:2] for r in BR.REQUESTS])
        _ORACLE_RUN["in"] = (ids, mask, px)
        _ORACLE_RUN["out"] = tiny.generate_beam(_t(ids), _t(px), _t(mask), BR.ORACLE_STEPS, BR.ORACLE_W,
                                                stop_token=None, num_return_sequences=BR.ORACLE_W, return_trace=True)
    return _ORACLE_RUN["in"], _ORACLE_RUN["out"]


def test_beam_search_against_the_oracle(tiny):
    """W = 3, stop_token None, on requests whose candidates the oracle keeps more than ragged_ref.MARGIN apart: over the
    steps that keep it the engine selects the oracle's tokens from the oracle's parents in the oracle's order, its
    scores within 2 TOL max|logit| per generated token; a request that keeps the margin to the end returns the
    oracle's hypotheses in the oracle's order."""
    _, out = _oracle_run(tiny)
    W, steps = BR.ORACLE_W, BR.ORACLE_STEPS
    for i, (_, _, n) in enumerate(BR.REQUESTS):
        ref = BR.reference(i)
        assert np.array_equal(out["tokens"][:n, i * W:(i + 1) * W].numpy(), ref["tokens"][:n]), i
        assert np.array_equal(out["parents"][:n, i * W:(i + 1) * W].numpy() - i * W, ref["parents"][:n]), i
        bound = 2 * TOL * float(np.abs(ref["logits"]).max())
        for t in range(n):
            d = np.abs(out["cum"][t, i * W:(i + 1) * W].numpy().astype(np.float64) - ref["cum"][t])
            print(f"request {i} step {t}: scores off by {d.max():.4f} of {(t + 1) * bound:.4f}")
            assert (d <= (t + 1) * bound).all(), (i, t, d)
        if n == steps:
            hyp, cum = BR.final_hypotheses(ref)
            assert out["sequences"][i] == hyp, (i, out["sequences"][i], hyp)
            assert out["beam_rows"][i].tolist() == [i * W + w for w in range(W)]
            d = np.abs(out["sum_logprobs"][i].numpy().astype(np.float64) - cum)
            assert (d <= steps * bound).all(), (i, d)


def test_hypotheses_rescored_by_the_oracle(tiny):
    """Every hypothesis of a 12-step, 3-beam search over pool requests 0 and 6, fed to the oracle token by token
    (score_ref.teacher_forced), has the summed log-probability generate_beam reports, within 2 TOL max|logit| per
    generated token: whatever the search chose, the score it reports is the model's score of that sequence, so its
    cache followed it."""
    import score_ref as S
    pool = [0, 6]
    ids, mask, px, _ = R.batch(2, rows=pool)
    out = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, 3, stop_token=None, num_return_sequences=3)
    for i, b in enumerate(pool):
        for j, hyp in enumerate(out["sequences"][i]):
            lgs = S.teacher_forced(b, hyp)
            want = sum(_lp64(lg[0], t) for lg, t in zip(lgs, hyp))
            bound = NEW * 2 * TOL * max(float(np.abs(lg).max()) for lg in lgs)
            d = abs(float(out["sum_logprobs"][i, j]) - want)
            print(f"request {b} hypothesis {j}: {d:.4f} of {bound:.4f}")
            assert d <= bound, (b, j, d, bound)


def test_best_hypothesis_scored_independently(tiny):
    """score() -- the tile-GEMM lm_head and the prefix-LM prefill, neither of which the decode step runs -- gives each
    request's best hypothesis the summed log-probability generate_beam reported, within the same per-token bound."""
    (ids, mask, px), out = _oracle_run(tiny)
    B, steps = len(BR.REQUESTS), BR.ORACLE_STEPS
    lens = mask.sum(-1)
    L = int(lens.max()) + steps
    s_ids = np.full((B, L), R.PAD, dtype=np.int64)
    s_mask = np.zeros((B, L), dtype=np.int64)
    s_type = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        n = int(lens[b])
        s_ids[b, :n] = ids[b, :n]
        s_ids[b, n:n + steps] = out["sequences"][b][0]
        s_mask[b, :n + steps] = 1
        s_type[b, n:n + steps] = 1
    sc = tiny.score(_t(s_ids), _t(px), _t(s_mask), _t(s_type))
    for b in range(B):
        bound = steps * 2 * TOL * float(np.abs(BR.reference(b)["logits"]).max())
        d = abs(float(sc["logprobs"][b, :steps].double().sum()) - float(out["sum_logprobs"][b, 0]))
        print(f"request {b}: score() differs by {d:.4f} of {bound:.4f}")
        assert d <= bound, (b, d, bound)


def test_stop_token_freezes_a_beam_and_length_penalty_ranks(tiny):
    """The stop token is an id the oracle's trace gives a non-best beam at step 2 or 3 (beam_ref.stop_choice): that
    beam's sequence ends there, its sum_logprobs is its traced cum at that step, its row emits pad afterwards, and the
    rankings under length_penalty 0, 1 and 2 are beam_ref.rank's of the same traced scores."""
    stop, s, w = BR.stop_choice()
    ids, mask, px = _pool_batch([BR.STOP_REQUEST])
    W, steps = BR.ORACLE_W, BR.STOP_STEPS
    seen = None
    for lp in (0.0, 1.0, 2.0):
        out = tiny.generate_beam(_t(ids), _t(px), _t(mask), steps, W, stop_token=stop, pad_token=PAD,
                                 length_penalty=lp, num_return_sequences=W, return_trace=True)
        tok, par = out["tokens"].numpy(), out["parents"].numpy()
        assert tok[s][w] == stop and stop not in tok[:s]
        frozen_cum = out["cum"][s][w]
        hyp = BR.backtrack(tok, par)
        mine = [r for r in range(W) if hyp[r][:s + 1] == BR.backtrack(tok[:s + 1], par[:s + 1], w)]
        assert len(mine) == 1, mine                             # the frozen beam is offered once per step
        r = mine[0]
        assert hyp[r][s + 1:] == [PAD] * (steps - s - 1)
        assert out["cum"][-1][r].view(torch.int32) == frozen_cum.view(torch.int32)
        want = BR.rank(hyp, out["cum"][-1].numpy(), W, stop, steps, lp)[0]
        assert out["beam_rows"][0].tolist() == [h[0] for h in want]
        assert out["sequences"][0] == [h[1] for h in want]
        assert np.allclose(out["scores"][0].numpy(), [h[2] for h in want], rtol=1e-6, atol=0)
        assert np.array_equal(out["sum_logprobs"][0].numpy(), np.array([h[3] for h in want], np.float32))
        k = out["beam_rows"][0].tolist().index(r)
        assert out["sequences"][0][k][-1] == stop and len(out["sequences"][0][k]) == s + 1
        assert out["sum_logprobs"][0, k].view(torch.int32) == frozen_cum.view(torch.int32)
        if seen is None:
            seen = (tok.copy(), par.copy())
        assert np.array_equal(seen[0], tok) and np.array_equal(seen[1], par)      # the penalty only re-ranks
    one = tiny.generate_beam(_t(ids), _t(px), _t(mask), steps, W, stop_token=stop, length_penalty=2.0)
    assert one["sequences"][0] == [want[0][1]] and tuple(one["scores"].shape) == (1, 1)


def test_all_beams_finished_ends_the_run(tiny):
    """When every beam has taken the stop token the host loop ends at its next check: one beam, the stop token the
    greedy run's second token, checked every step."""
    ids, px = R.request(0)
    mask = np.ones_like(ids)
    g = tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=None)[0].tolist()
    cut = g.index(g[1]) + 1
    out = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, 1, stop_token=g[1], return_trace=True, check_every=1)
    assert out["sequences"][0][0] == g[:cut]
    assert out["tokens"].shape[0] == cut, "the run went on after its only beam had finished"
    # checked every 8 steps (the default for more than one row) the frozen rows emit pad until then
    out = tiny.generate_beam(_t(ids), _t(px), _t(mask), NEW, 2, stop_token=g[1], return_trace=True,
                             num_return_sequences=2)
    assert out["sequences"][0][0][-1] == g[1] or len(out["sequences"][0][0]) == NEW


def test_model_level_generate_beam(tiny):
    """PaliGemmaForConditionalGeneration.generate_beam returns its engine's result, and generate is untouched."""
    from oracle import configs as ocfg, synth
    from modeling_paligemma import PaliGemmaConfig, PaliGemmaForConditionalGeneration
    m = PaliGemmaForConditionalGeneration(PaliGemmaConfig(**ocfg.TINY))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.generate_state_dict(ocfg.TINY).items()}, strict=False)
    m.tie_weights()
    m = m.to("cuda").eval()
    ids, mask, px, _ = R.batch(2, rows=[0, 4])
    got = m.generate_beam(_t(ids), _t(px), _t(mask), max_new_tokens=6, num_beams=3, num_return_sequences=2,
                          stop_token=None)
    want = m.engine(_t(ids).device).generate_beam(_t(ids), _t(px), _t(mask), 6, 3, num_return_sequences=2,
                                                  stop_token=None)
    assert got["sequences"] == want["sequences"] and torch.equal(got["scores"], want["scores"])
    assert len(got["sequences"]) == 2 and all(len(s) == 2 and all(len(h) == 6 for h in s) for s in got["sequences"])
    a = m.generate(_t(ids), _t(px), _t(mask), max_new_tokens=6, stop_token=None)
    b = m.engine(_t(ids).device).generate(_t(ids), _t(px), _t(mask), 6, stop_token=None)
    assert torch.equal(a, b)
    assert [s[0] for s in m.generate_beam(_t(ids), _t(px), _t(mask), max_new_tokens=6, num_beams=1,
                                          stop_token=None)["sequences"]] == a.tolist()
