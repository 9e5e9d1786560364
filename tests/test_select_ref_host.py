"""The sampler contract checker (tests/select_ref.py) against the reference sampler, without a device: the
reference's own draws stay inside the tolerance, and a draw of the kind the kernel's fallback produced (the last
kept token for a uniform from the middle of the CDF) is flagged."""
import numpy as np

import select_ref as R
from oracle import paligemma_oracle as O


def _row(V, seed):
    return (np.random.default_rng(seed).standard_normal(V) * 3).astype(np.float32)


def _oracle_kept(x, T, P):
    probs = O.softmax_lastdim((x[None] / np.float32(T)).astype(np.float32))
    ps, idx = O.top_p_filter(probs, P)
    kept = np.zeros(x.shape[0], dtype=bool)
    kept[idx[0][ps[0] > 0]] = True
    return kept


def test_reference_draws_pass_and_a_planted_fallback_draw_is_flagged():
    V, T, P, n = 1000, 0.8, 0.9, 10000
    x = _row(V, 5)
    assert (x.max() - x.min()) / T <= 32
    ref = R.TopPRow(x, T, P)
    kept = _oracle_kept(x, T, P)
    assert ref.check_kept(kept) == []
    rng = np.random.default_rng(6)
    u = rng.random(n, dtype=np.float32)
    u[:3] = [0.0, np.nextafter(np.float32(1), np.float32(0)), 0.5]
    ids = O.sample_top_p(np.broadcast_to(x, (n, V)), T, P, u)[:, 0]
    bad = ref.check_draw(u, ids, kept)
    assert not bad.any(), (int(bad.sum()), u[bad][:5], ids[bad][:5])
    # the fallback defect: the last kept token of the vocabulary for a u in the middle of the CDF
    last = int(np.nonzero(kept)[0].max())
    F = ref.cdf(kept)
    assert F[last] - 0.5 > 100 * ref.tol          # the planted draw is far outside the allowance
    assert ref.check_draw(np.float32(0.5), last, kept).all()
    # and the checker's other refusals: a token outside the kept set, an id outside the vocabulary
    out = int(np.nonzero(~kept)[0][0])
    assert ref.check_draw(np.float32(F[out]), out, kept).all()
    assert ref.check_draw(np.float32(0.5), V, kept).all() and ref.check_draw(np.float32(0.5), -1, kept).all()


def test_kept_set_rules():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 0.0], dtype=np.float32)
    ref = R.TopPRow(x, 1.0, 0.0)
    assert ref.K.tolist() == [False, True, True, False, False, False]      # top_p = 0: the maximal tie group
    assert ref.check_kept(ref.K) == []
    assert ref.check_kept([False, True, False, False, False, False])       # a split tie group
    assert ref.check_kept([False] * 6)                                     # nothing kept
    full = R.TopPRow(x, 1.0, 1.0)
    assert full.K.tolist() == [True, True, True, False, True, True]        # top_p = 1: everything but -inf
    assert full.check_kept([True] * 6)                                     # -inf kept
    # a token far on the wrong side of the cut is refused, one within the slack is not
    mid = R.TopPRow(x, 1.0, 0.5)
    assert mid.check_kept(full.K)
    near = R.TopPRow(x, 1.0, float(mid.before[4]) - 1e-6)                  # the cut lands just before token 4
    assert not near.K[4] and near.check_kept(near.K | (np.arange(6) == 4)) == []


def test_ulp_window_and_chunk_starts():
    w = R.ulp_window([0.5, 0.0, 1.0], 2)
    assert w.dtype == np.float32 and (w >= 0).all() and (w < 1).all()
    h = np.float32(0.5)
    assert set(w.tolist()) >= {float(np.nextafter(h, np.float32(0))), 0.5, float(np.nextafter(h, np.float32(1))), 0.0}
    ref = R.TopPRow(_row(8197, 1), 1.0, 1.0)
    c = ref.chunk_starts()
    assert c.shape == (910,) and np.isclose(c[0], ref.p[:9].sum())         # ceil(8197 / 9) = 911 non-empty chunks
    assert R.draw_tol(8197) == 20 * 2.0 ** -24 + 2.0 ** -19
