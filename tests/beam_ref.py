"""References for the beam-search tests (tests/test_beam_host.py, tests/test_beam_gpu.py); no GPU code.

The semantics are PaliGemmaEngine.generate_beam's ("Beam search"): B prompts of W beams, rows bW .. bW + W - 1
prompt b's group; a hypothesis's score is the sum of its tokens' log-probabilities; a live parent p offers (p, t) for
every token t, a finished parent only (p, pad) with its score unchanged; the best W candidates per group are kept, best
first, ties to the lower (p, t); a NaN score loses to every comparable one; a row of nothing but -inf scores -inf.

  select      one selection step in float64 numpy
  check_select  the tolerance-aware comparison of a float32 selection with it
  gather      the KV reorder on numpy copies of the four cache layouts (dec_koff / dec_voff re-derived from the layout
              description in csrc/attn_common.h)
  backtrack, rank   hypotheses from the two histories, and the final ranking under a length penalty
  beam_search   the whole search on the oracle, teacher-forced through forks of its KVCache

The oracle requests of the engine tests (REQUESTS) are pool requests of tests/ragged_ref.py under seeds chosen on the
oracle alone (`python tests/beam_ref.py search`): a seed qualifies for n steps when every one of the first n steps of a
W = 3 search keeps its candidates apart by more than ragged_ref.MARGIN -- the gap between the W-th kept and the best
dropped candidate, and the gaps between the kept candidates' scores -- so that two correct bf16 implementations cannot
legitimately disagree on a hypothesis or on its rank.  Four gaps per step above 0.1, with TINY's 300 logits spanning
+-2.4, are rare: over seeds 0..5999 of every pool request no seed keeps the margin for three steps, two requests have
one that keeps it for two, and every request has one for the first step (the search prints, per request, the most
steps any seed kept and the first seed that did).  The margin was not shrunk; the steps were: ORACLE_STEPS = 2, and the
third request is compared over its first step only.  What the longer runs decide is checked without the oracle's
margins: every selection against float64 on the engine's own logits, the gather by the teacher-forced bit comparison,
and every returned hypothesis re-scored by the oracle, teacher-forced.
"""
import numpy as np

import ragged_ref as R

ORACLE_W, ORACLE_STEPS = 3, 2
# (pool request, seed, steps that keep the margin): `python tests/beam_ref.py search` prints these
REQUESTS = [(6, 4814, 2), (5, 2712, 2), (0, 243, 1)]
# The frozen-beam test's request (`python tests/beam_ref.py search-stop`): its stop token comes from step 2 or 3 of the
# oracle's trace, so the engine has to follow the oracle that far.  No seed keeps MARGIN for three steps; this one
# keeps every gap of its first four steps above STOP_FLOOR = 0.04, the floor ragged_ref's own seeds hold for greedy ids
# (two correct bf16 implementations differ by about 1e-3 of the logits' scale, 2.4).  Everything that test asserts
# beyond "the stop token is taken there" is checked against the engine's own trace.
STOP_FLOOR = 0.04
STOP_REQUEST = (0, 518)
STOP_STEPS = 6


# --------------------------------------------------------------------------------------------------- selection
def row_scores(x, cum_p):
    """float64 scores cum_p + log_softmax(x) of one live parent's V candidates."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).any():
        return np.full(x.shape, np.nan)
    m = x.max()
    if m == -np.inf:
        return np.full(x.shape, -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(cum_p) + ((x - m) - np.log(np.exp(x - m).sum()))


def _order(scores, p, t):
    """Indices sorting candidates best first: comparable scores descending, NaN last, ties to the lower (p, t)."""
    nan = np.isnan(scores)
    return np.lexsort((t, p, np.where(nan, 0.0, -scores), nan))


def candidates(logits, cum, finished, W, pad, g, keep=None):
    """(scores, parents, tokens) of group g's candidates, float64 / int64 arrays.  keep: only each live parent's best
    `keep` (a row's scores rise with its logits, so the group's best n <= keep candidates are among them)."""
    V = logits.shape[1]
    sc, pp, tt = [], [], []
    for p in range(g * W, g * W + W):
        if finished[p]:
            sc.append(np.array([float(cum[p])])); pp.append(np.array([p])); tt.append(np.array([pad]))
            continue
        s, t = row_scores(logits[p], cum[p]), np.arange(V)
        if keep is not None and keep < V:
            t = _order(s, np.zeros(V, np.int64), t)[:keep]
            s = s[t]
        sc.append(s); pp.append(np.full(len(t), p)); tt.append(t)
    return np.concatenate(sc), np.concatenate(pp), np.concatenate(tt)


def select(logits, cum, finished, W, stop, pad):
    """One selection step: (ids int64, parent int64 (global rows), cum float64, finished int, all_finished) for rows =
    B * W; stop None or negative: nothing finishes.  With `gaps` see select_gaps."""
    logits = np.asarray(logits)
    rows = logits.shape[0]
    ids, par = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    ncum, nfin = np.zeros(rows, np.float64), np.zeros(rows, np.int64)
    for g in range(rows // W):
        sc, pp, tt = candidates(logits, cum, finished, W, pad, g, keep=W)
        best = _order(sc, pp, tt)[:W]
        for j, c in enumerate(best):
            o = g * W + j
            ids[o], par[o], ncum[o] = tt[c], pp[c], sc[c]
            nfin[o] = int(bool(finished[pp[c]]) or (stop is not None and stop >= 0 and tt[c] == stop))
    return ids, par, ncum, nfin, bool(nfin.all())


def select_gaps(logits, cum, finished, W, pad):
    """The smallest of, over the groups: the gaps between consecutive kept scores and the gap between the W-th kept and
    the best dropped candidate (inf where there is none)."""
    worst = np.inf
    for g in range(np.asarray(logits).shape[0] // W):
        sc, pp, tt = candidates(logits, cum, finished, W, pad, g, keep=W + 1)
        o = _order(sc, pp, tt)[:W + 1]
        s = sc[o]
        with np.errstate(invalid="ignore"):
            d = s[:-1] - s[1:]
        d = d[~np.isnan(d)]
        if d.size:
            worst = min(worst, float(d.min()))
    return worst


def check_select(logits, cum, finished, W, stop, pad, got_ids, got_parent, got_cum, got_fin, rtol):
    """A float32 selection against float64, tolerant of the log-sum-exp's rounding: every returned candidate is a legal
    one, no candidate twice, its float64 score is at least the W-th best float64 score minus eps, the returned cum is
    within eps of it, the returned order is non-increasing, the finished flag is the parent's or set by `stop`.
    eps = rtol * max(1, |score|): the bound pg_token_logprob's test holds the same arithmetic to (PROBS_RTOL)."""
    logits = np.asarray(logits)
    rows, V = logits.shape
    for g in range(rows // W):
        sc, pp, tt = candidates(logits, cum, finished, W, pad, g, keep=W)
        kth = sc[_order(sc, pp, tt)[W - 1]]
        rows64 = {}                                      # a live parent's float64 scores, computed when first asked for
        seen = set()
        prev = None
        for j in range(W):
            o = g * W + j
            p, t, c = int(got_parent[o]), int(got_ids[o]), float(got_cum[o])
            assert g * W <= p < g * W + W and 0 <= t < V, (g, j, p, t)
            assert (p, t) not in seen, (g, j, p, t)
            seen.add((p, t))
            if finished[p]:
                assert t == pad and c == float(cum[p]), (g, j, p, t, c)
                s = float(cum[p])
            else:
                if p not in rows64:
                    rows64[p] = row_scores(logits[p], cum[p])
                s = float(rows64[p][t])
            eps = rtol * max(1.0, abs(s)) if np.isfinite(s) else 0.0
            if np.isnan(kth):
                pass                                    # fewer than W comparable candidates: any legal one fills in
            elif np.isinf(s) or np.isnan(s):
                assert np.isinf(kth) and kth < 0 and (np.isnan(s) or s < 0), (g, j, s, kth)
            else:
                assert s >= kth - eps, (g, j, p, t, s, kth)
            if np.isnan(s):
                assert np.isnan(c), (g, j, c)
            elif np.isinf(s):
                assert c == s, (g, j, c, s)
            else:
                assert abs(c - s) <= eps, (g, j, c, s)
            if prev is not None and not np.isnan(c):
                assert not np.isnan(prev) and c <= prev, (g, j, prev, c)
            prev = c
            want_fin = int(bool(finished[p]) or (stop is not None and stop >= 0 and t == stop))
            assert int(got_fin[o]) == want_fin, (g, j, p, t)


# --------------------------------------------------------------------------------------------------- KV reorder
def dec_koff(k, d, D):
    """Element offset of (key k, dim d) in a (row, kv head)'s decode-order K copy.  Per 32-key block:
    [half h][D/8 chunks][16 MFMA rows][8 dims]; row r of half h is key 8 (r / 4) + 4 h + r % 4."""
    blk, kk = k >> 5, k & 31
    h, r = (kk >> 2) & 1, ((kk >> 3) << 2) | (kk & 3)
    return ((((blk * 2 + h) * (D >> 3) + (d >> 3)) * 16 + r) * 8 + (d & 7))


def dec_voff(k, d, D):
    """... in its decode-order V copy.  Per 32-key block: [D/16 d-tiles][4 key groups g][16 dims][8 keys 8g .. 8g + 7]."""
    blk, kk = k >> 5, k & 31
    return ((((blk * (D >> 4) + (d >> 4)) * 4 + (kk >> 3)) * 16 + (d & 15)) * 8 + (kk & 7))


def dec_maps(Smax, D):
    """(koff, voff) int64 [Smax][D]: where (position, dim) sits in a head's Smax * D decode-order elements."""
    k, d = np.meshgrid(np.arange(Smax), np.arange(D), indexing="ij")
    return dec_koff(k, d, D), dec_voff(k, d, D)


def pack_dec(k, vt, Hkv):
    """(kd, vd) [layers][rows][Hkv][Smax * D] from canonical k [layers][rows][Smax][Hkv * D] and vt
    [layers][rows][Hkv * D][Smax]."""
    nl, rows, S, kvd = k.shape
    D = kvd // Hkv
    ko, vo = dec_maps(S, D)
    kd = np.zeros((nl, rows, Hkv, S * D), k.dtype)
    vd = np.zeros((nl, rows, Hkv, S * D), k.dtype)
    for h in range(Hkv):
        kd[:, :, h, ko] = k[:, :, :, h * D:(h + 1) * D]
        vd[:, :, h, vo] = vt[:, :, h * D:(h + 1) * D, :].transpose(0, 1, 3, 2)
    return kd, vd


def gather(k, vt, kd, vd, parent, base, length, Hkv):
    """The contract of pg_kv_beam_gather on numpy arrays (any dtype; kd / vd as pack_dec makes them): new arrays in
    which positions [base[r], length[r]) of row r are row parent[r]'s old ones, in all four layouts."""
    nk, nvt, nkd, nvd = k.copy(), vt.copy(), kd.copy(), vd.copy()
    S, D = k.shape[2], k.shape[3] // Hkv
    ko, vo = dec_maps(S, D)
    for r, p in enumerate(parent):
        lo, hi = int(base[r]), int(length[r])
        if p == r or hi <= lo:
            continue
        nk[:, r, lo:hi] = k[:, p, lo:hi]
        nvt[:, r, :, lo:hi] = vt[:, p, :, lo:hi]
        for idx, new, old in ((ko, nkd, kd), (vo, nvd, vd)):
            sel = idx[lo:hi].reshape(-1)
            new[:, r][:, :, sel] = old[:, p][:, :, sel]
    return nk, nvt, nkd, nvd


def position_masks(Smax, D, lo, hi):
    """Boolean masks over a head's Smax * D decode-order elements: those of positions [lo, hi) in K and in V order."""
    ko, vo = dec_maps(Smax, D)
    mk, mv = np.zeros(Smax * D, bool), np.zeros(Smax * D, bool)
    mk[ko[lo:hi].reshape(-1)] = True
    mv[vo[lo:hi].reshape(-1)] = True
    return mk, mv


# --------------------------------------------------------------------------------------------------- hypotheses
def backtrack(hist_tok, hist_parent, row=None):
    """The token lists of the hypotheses ending in each row (or in `row`) after the last step of [steps][rows]
    histories; parents are global row indices."""
    hist_tok, hist_parent = np.asarray(hist_tok), np.asarray(hist_parent)

    def one(r):
        out = []
        for t in range(hist_tok.shape[0] - 1, -1, -1):
            out.append(int(hist_tok[t][r]))
            r = int(hist_parent[t][r])
        return out[::-1]
    return one(row) if row is not None else [one(r) for r in range(hist_tok.shape[1])]


def ancestry(hist_parent, row):
    """The row a final row's hypothesis occupied after each step: rows[t] for t = 0 .. steps - 1 (rows[-1] == row)."""
    hist_parent = np.asarray(hist_parent)
    out = [row]
    for t in range(hist_parent.shape[0] - 1, 0, -1):
        out.append(int(hist_parent[t][out[-1]]))
    return out[::-1]


def rank(tokens, cum, W, stop, max_new_tokens, length_penalty, n_return=None):
    """Final ranking per prompt: hypotheses = backtracked token lists of all rows, cum their sums.  Returns per prompt
    a list of (beam index, sequence cut at its stop token, score, sum), best first: score = sum / n ** length_penalty,
    n = tokens up to and including the stop token, or max_new_tokens for an unfinished beam; ties to the lower beam."""
    out = []
    for g in range(len(tokens) // W):
        hyp = []
        for w in range(W):
            toks = list(tokens[g * W + w])
            if stop is not None and stop in toks:
                toks = toks[: toks.index(stop) + 1]
                n = len(toks)
            else:
                n = max_new_tokens
            c = float(cum[g * W + w])
            hyp.append((w, toks, c / float(n) ** float(length_penalty), c))
        hyp.sort(key=lambda h: (h[2] != h[2], -h[2] if h[2] == h[2] else 0.0))      # stable: ties keep beam order
        out.append(hyp[: n_return or W])
    return out


# --------------------------------------------------------------------------------------------------- the oracle
def _fork(kv):
    from oracle import paligemma_oracle as O
    new = O.KVCache()
    new.k_cache, new.v_cache = list(kv.k_cache), list(kv.v_cache)     # update() concatenates: the arrays are never
    return new                                                          # written in place, so a fork shares them


def beam_search(b, W=ORACLE_W, steps=ORACLE_STEPS, stop=None, pad=R.PAD, seed=None, orc=None, min_gap=None):
    """Beam search on the oracle for pool request b: the prompt through forward() once, then every live beam's token
    one at a time through its own fork of the KVCache (score_ref.teacher_forced's way).  Returns {"tokens", "parents"
    int64 [steps][W], "cum" float64 [steps][W], "logits" [steps][W][V] the logits each selection read, "gaps" [steps]
    select_gaps per step}.  min_gap: give up at the first step whose gap is not above it, returning that step's index."""
    from oracle import paligemma_oracle as O
    orc = R.oracle() if orc is None else orc
    ids, px = R.request(b, seed)
    mask = np.ones_like(ids)
    kv = O.KVCache()
    lg = orc.forward(ids, px, mask, kv, logits_rows=slice(-1, None))["logits"][:, -1, :]
    caches = [_fork(kv) for _ in range(W)]
    logits = np.repeat(np.asarray(lg, np.float32), W, axis=0)
    cum = np.full(W, -np.inf); cum[0] = 0.0
    fin = np.zeros(W, np.int64)
    out = {"tokens": [], "parents": [], "cum": [], "logits": [], "gaps": []}
    for s in range(steps):
        gap = select_gaps(logits, cum, fin, W, pad)
        if min_gap is not None and not gap > min_gap:
            return s
        tok, par, cum, fin, _ = select(logits, cum, fin, W, stop, pad)
        out["tokens"].append(tok); out["parents"].append(par); out["cum"].append(cum.copy())
        out["logits"].append(logits.copy()); out["gaps"].append(gap)
        if s == steps - 1:
            break
        caches = [_fork(caches[p]) for p in par]
        mask = np.concatenate([mask, np.ones((1, 1), dtype=mask.dtype)], axis=-1)
        logits = np.zeros_like(logits)
        for r in range(W):
            if not fin[r]:                            # a finished beam's logits are never read
                cur = np.array([[int(tok[r])]], dtype=np.int64)
                logits[r] = orc.forward(cur, px, mask, caches[r], logits_rows=slice(-1, None))["logits"][0, -1, :]
    return {k: np.array(v) for k, v in out.items()}


_REF = {}


def reference(i):
    """beam_search of REQUESTS[i] over ORACLE_STEPS steps (computed once); only its first REQUESTS[i][2] steps keep the
    margin."""
    if i not in _REF:
        b, seed, _ = REQUESTS[i]
        _REF[i] = beam_search(b, seed=seed)
    return _REF[i]


def stop_reference():
    """beam_search of STOP_REQUEST over STOP_STEPS steps with no stop token (computed once)."""
    if "stop" not in _REF:
        _REF["stop"] = beam_search(STOP_REQUEST[0], steps=STOP_STEPS, seed=STOP_REQUEST[1])
    return _REF["stop"]


def stop_choice(ref=None):
    """The stop token of the frozen-beam test: the id the oracle's trace of STOP_REQUEST gives to a non-best beam at
    step 2 or 3, which no beam holds before that step and no other beam takes at it (so that beam is the first, and
    the only one, to finish there).  Returns (token, step, beam), or None when the trace offers none."""
    ref = stop_reference() if ref is None else ref
    for s in (2, 3):
        if s >= len(ref["tokens"]):
            break
        earlier = set(ref["tokens"][:s].reshape(-1).tolist())
        for w in range(1, ORACLE_W):
            t = int(ref["tokens"][s][w])
            if t not in earlier and list(ref["tokens"][s]).count(t) == 1 and t not in (R.PAD, R.BOS, R.IMAGE_ID):
                return t, s, w
    return None


def final_hypotheses(ref):
    """(token lists per final row, final cum) of a beam_search result."""
    return backtrack(ref["tokens"], ref["parents"]), ref["cum"][-1]


if __name__ == "__main__":     # `search [pool rows]`, `search-stop [pool rows]`: the searches behind REQUESTS and
    import sys                 # STOP_REQUEST; otherwise each request's trace and gaps
    pool = [int(a) for a in sys.argv[2:]] or [0, 3, 9, 6, 4, 13, 10, 14, 5, 11]
    if sys.argv[1:2] == ["search"]:
        for b in pool:
            best = (-1, None)                          # (steps that kept the margin, the first seed that reached them)
            for seed in range(6000):
                ref = beam_search(b, seed=seed, min_gap=R.MARGIN)
                if isinstance(ref, dict):
                    best = (ORACLE_STEPS, seed)
                    break
                if ref > best[0]:
                    best = (ref, seed)
            print(b, "steps", best[0], "seed", best[1], flush=True)
    elif sys.argv[1:2] == ["search-stop"]:
        for b in pool:
            for seed in range(2000):
                ref = beam_search(b, steps=4, seed=seed, min_gap=STOP_FLOOR)
                if isinstance(ref, dict) and stop_choice(ref) is not None:
                    print(b, "seed", seed, "stop", stop_choice(ref), "gaps", " ".join(f"{g:.3f}" for g in ref["gaps"]),
                          flush=True)
                    break
    else:
        for i, (b, seed, _) in enumerate(REQUESTS):
            ref = reference(i)
            print(i, b, seed, "gaps", " ".join(f"{g:.3f}" for g in ref["gaps"]))
            print("   tokens", ref["tokens"].tolist(), "parents", ref["parents"].tolist())
        ref = stop_reference()
        print("stop", STOP_REQUEST, stop_choice(), "gaps", " ".join(f"{g:.3f}" for g in ref["gaps"]))
        print("   tokens", ref["tokens"].tolist(), "parents", ref["parents"].tolist())
