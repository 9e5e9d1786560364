"""Inputs and oracle references for the ragged-batch tests (tests/test_ragged_gpu.py); no GPU code.

A pool of 17 TINY requests of different prompt lengths: 16 image tokens (id 299), <bos> (2), seeded random text ids in
3..298, and one seeded random image each.  Row b of a batch of B is the pool's request b, right-padded with the pad
id 0 to the batch's longest prompt.  The contract under test is that each row generates what the oracle generates for
that request ALONE, unpadded, at B = 1 (oracle.generate: the reference's loop), so the references are computed once
per request and shared by every test.

The lengths, by the rules the tests need (a batch of the first B rows keeps them for B >= 3):
  19            the shortest rows hold one or two text tokens (18 = one, row 3), and 19 + 16 decoded steps crosses 32
  192, 193      a multiple of 64, and that plus 1; both >= two 64-key blocks longer than the shortest
  18, 64, 65    one text token; one 64-key block exactly, and one key more
  31, 128, ...  a row that reaches 32 keys with its first decoded token, whole 32- / 64-key blocks, and fillers
"""
import numpy as np

LENS = [19, 192, 193, 18, 64, 65, 31, 128, 129, 20, 47, 96, 150, 33, 63, 160, 191]
N_IMG, IMAGE_ID, BOS, PAD = 16, 299, 2, 0
STEPS = 16
# Greedy ids are required equal where the oracle's top-1 / top-2 margin exceeds this (logit units; TINY's logits span
# about +-2.4, and with an arbitrary seed its margin falls below 0.01 at about one step in ten)
MARGIN = 0.1
# One seed per request (text ids and image), searched (`python tests/ragged_ref.py search`) for a large smallest margin
# over the oracle's own 16 free-running steps, so that free-running ids can be compared at all: every request stays
# above 0.04.  (The seeds with the very largest margins make the model repeat one token; for the short requests 0, 3,
# 4 and 6 the best seed with at least five distinct tokens was taken instead.)  Two correct bf16 implementations -- or
# one at two batch sizes -- differ by about 1e-3 of the logits' scale, far below these margins.
SEEDS = [30, 1236, 1826, 367, 145, 21, 115, 1109, 3603, 176, 24, 65, 4219, 4993, 2969, 1406, 5801]


def request(b: int, seed=None):
    """(input_ids int64 [1][len_b], pixel_values fp32 [1][3][56][56]) of pool request b."""
    n = LENS[b]
    seed = SEEDS[b] if seed is None else seed
    rng = np.random.default_rng([seed, b])
    text = rng.integers(3, 299, size=n - N_IMG - 1)
    ids = np.concatenate([np.full(N_IMG, IMAGE_ID), [BOS], text]).astype(np.int64)[None]
    px = rng.uniform(-1.0, 1.0, size=(1, 3, 56, 56)).astype(np.float32)
    return ids, px


def batch(B: int, rows=None):
    """(input_ids [B][L] right-padded with PAD, attention_mask [B][L], pixel_values [B][3][56][56], lens) of the pool
    requests `rows` (default the first B)."""
    rows = list(range(B)) if rows is None else list(rows)
    reqs = [request(b) for b in rows]
    lens = [LENS[b] for b in rows]
    L = max(lens)
    ids = np.full((len(rows), L), PAD, dtype=np.int64)
    mask = np.zeros((len(rows), L), dtype=np.int64)
    for i, (r, _) in enumerate(reqs):
        ids[i, :lens[i]] = r[0]
        mask[i, :lens[i]] = 1
    return ids, mask, np.concatenate([p for _, p in reqs]), lens


_ORACLE = {}
_REF = {}


def oracle():
    if "o" not in _ORACLE:
        from oracle import configs as ocfg, synth, paligemma_oracle as O
        _ORACLE["o"] = O.PaliGemmaOracle(ocfg.TINY, synth.generate_state_dict(ocfg.TINY), recompute_vision=False)
    return _ORACLE["o"]


def reference(b: int, seed=None):
    """(greedy ids [STEPS], logits [STEPS][1][V], margins [STEPS]) of the oracle's free-running greedy loop on pool
    request b alone, unpadded (computed once)."""
    key = (b, seed)
    if key not in _REF:
        from oracle import paligemma_oracle as O
        ids, px = request(b, seed)
        out, logits = O.generate(oracle(), ids, px, np.ones_like(ids), STEPS, stop_token=None, record_logits=True)
        top = [np.sort(lg[0])[::-1] for lg in logits]
        _REF[key] = (out, logits, np.array([t[0] - t[1] for t in top]))
    return _REF[key]


if __name__ == "__main__":     # each request's oracle ids and per-step margins; `search`: the seed search behind SEEDS
    import sys
    if sys.argv[1:] == ["search"]:
        for b in range(len(LENS)):
            best = (-1.0, None)
            for seed in range(6000):
                m = float(reference(b, seed)[2].min())
                best = max(best, (m, seed))
                if len(set(reference(b, seed)[0])) >= 5 and m > 0.04:
                    print(b, LENS[b], "varied:", (m, seed), flush=True)
                del _REF[(b, seed)]
                if m > MARGIN + 0.005:
                    break
            print(b, LENS[b], best, flush=True)
    else:
        for b in range(len(LENS)):
            out, _, m = reference(b)
            print(b, LENS[b], out, f"min {m.min():.3f}:", " ".join(f"{x:.3f}" for x in m), flush=True)
