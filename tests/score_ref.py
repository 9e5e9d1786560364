"""Inputs and oracle references for the scoring tests (tests/test_score_gpu.py); no GPU code.

A scoring batch is the first B pool requests of tests/ragged_ref.py, each followed by an answer: row b is
[request b's ids | answer b | pad].  Two kinds of answer:

  greedy     the oracle's own 16 free-running greedy tokens of request b (ragged_ref.reference), whose per-step
             logits are the reference already: logits[t] is what the model predicts after answer tokens 0 .. t - 1
  arbitrary  seeded random ids of the lengths SUFFIX_LENS (so rows differ in prefix AND answer length), fed to
             PaliGemmaOracle.forward one token at a time through its KVCache -- the oracle used as a library, its
             decode path being the only causal one it has (its prefill mask is all zeros)

Either way the reference of row b is a list of S_b logits rows [1][V]; row t scores answer token t.

The arbitrary answers' seeds are chosen on the oracle alone (`python tests/score_ref.py search`).  TINY's logits span
about +-2.4, and a random answer can drive a step whose logits the oracle's own bf16-operand run (bf16_operands: fp32
arithmetic on bf16-rounded operands, the least any bf16 implementation deviates) already misses by the 3e-2 logits
bound: such a step measures the request's conditioning, not the kernels.  A seed is taken when that run stays within
EMU_MAX = 2e-2 = 2/3 of the bound at every step, the first such seed counting up from 0; the tests then hold the
engine, a second bf16 implementation with its own summation order and bf16 activations, to the full 3e-2."""
import numpy as np

import ragged_ref as R

SUFFIX_LENS = [16, 1, 7, 2, 16, 3, 9, 5]
EMU_MAX = 2e-2
SEEDS = [4, 0, 0, 0, 2, 0, 0, 0]
_REF = {}


def suffix(b: int, seed=None) -> np.ndarray:
    """The arbitrary answer of pool request b: SUFFIX_LENS[b] seeded random text ids in 3..298."""
    rng = np.random.default_rng([977, b, SEEDS[b] if seed is None else seed])
    return rng.integers(3, 299, size=SUFFIX_LENS[b]).astype(np.int64)


def teacher_forced(b: int, answer, orc=None):
    """Oracle logits [S][1][V] for `answer` after pool request b: the prompt through forward() once, then the answer's
    tokens one at a time through the same KVCache (the last token is scored but never fed)."""
    from oracle import paligemma_oracle as O
    orc = R.oracle() if orc is None else orc
    ids, px = R.request(b)
    kv = O.KVCache()
    mask = np.ones_like(ids)
    out = []
    cur = ids
    for t in range(len(answer)):
        res = orc.forward(cur, px, mask, kv, logits_rows=slice(-1, None))
        out.append(res["logits"][:, -1, :].copy())
        cur = np.array([[int(answer[t])]], dtype=np.int64)
        mask = np.concatenate([mask, np.ones((1, 1), dtype=mask.dtype)], axis=-1)
    return out


def reference(b: int):
    """(answer ids, logits [S_b][1][V]) of the arbitrary answer of pool request b (computed once)."""
    if b not in _REF:
        ans = suffix(b)
        _REF[b] = (ans, teacher_forced(b, ans))
    return _REF[b]


def batch(answers):
    """(input_ids, attention_mask, token_type_ids [B][L], pixel_values [B][3][56][56], prefix lengths) of the pool
    requests 0 .. B - 1, request b followed by answers[b], right-padded with the pad id."""
    B = len(answers)
    reqs = [R.request(b) for b in range(B)]
    prefix = [R.LENS[b] for b in range(B)]
    L = max(p + len(a) for p, a in zip(prefix, answers))
    ids = np.full((B, L), R.PAD, dtype=np.int64)
    mask = np.zeros((B, L), dtype=np.int64)
    types = np.zeros((B, L), dtype=np.int64)
    for b, ((r, _), a) in enumerate(zip(reqs, answers)):
        n = prefix[b] + len(a)
        ids[b, :prefix[b]] = r[0]
        ids[b, prefix[b]:n] = np.asarray(a, dtype=np.int64)
        mask[b, :n] = 1
        types[b, prefix[b]:n] = 1
    return ids, mask, types, np.concatenate([p for _, p in reqs]), prefix


def log_softmax64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def emulated_distance(b: int, answer) -> float:
    """Largest scaled max error, over the answer's steps, of the oracle on bf16-rounded operands from the fp32 oracle."""
    from oracle import paligemma_oracle as O
    ref = teacher_forced(b, answer)
    with O.bf16_operands():
        emu = teacher_forced(b, answer)
    return max(float(np.abs(e.astype(np.float64) - r).max() / np.abs(r).max()) for e, r in zip(emu, ref))


if __name__ == "__main__":     # `search`: the seed search behind SEEDS; otherwise each row's distance under its seed
    import sys
    for b in range(len(SUFFIX_LENS)):
        if sys.argv[1:] == ["search"]:
            seed = 0
            while emulated_distance(b, suffix(b, seed)) >= EMU_MAX:
                seed += 1
            print(b, "seed", seed, flush=True)
        else:
            print(b, SEEDS[b], f"{emulated_distance(b, suffix(b)):.4f}", flush=True)
