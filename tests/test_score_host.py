"""Scoring given answers (PaliGemmaEngine.score): the checks that need no GPU.

The layout rule of a scoring batch (engine.score_spans: [prefix | suffix | pad] per row), raised by score() before any
launch; the argument checks of pg_attention_prefix and pg_token_logprob (hipErrorInvalidValue before any HIP call, so
the library answers without a device); PaliGemmaProcessor.batch(..., suffixes=...) on the offline tokenizer."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1


def _rows(spec, L):
    """(mask, type ids) [B][L] from (prefix, suffix) lengths per row."""
    mask = torch.zeros(len(spec), L, dtype=torch.int64)
    types = torch.zeros(len(spec), L, dtype=torch.int64)
    for b, (p, s) in enumerate(spec):
        mask[b, :p + s] = 1
        types[b, p:p + s] = 1
    return mask, types


def test_score_spans_accepts_prefix_suffix_pad_only():
    from pghip.engine import PaliGemmaEngine
    mask, types = _rows([(5, 3), (1, 1), (2, 6), (7, 1)], 8)
    prefix, lens = PaliGemmaEngine.score_spans(mask, types)
    assert prefix.tolist() == [5, 1, 2, 7] and lens.tolist() == [8, 2, 8, 8]
    prefix, lens = PaliGemmaEngine.score_spans(mask.bool(), types.bool())
    assert prefix.tolist() == [5, 1, 2, 7] and lens.tolist() == [8, 2, 8, 8]

    def bad(mask, types, what):
        with pytest.raises(ValueError, match=what):
            PaliGemmaEngine.score_spans(mask, types)

    m, t = _rows([(5, 3), (4, 2)], 8)
    t2 = t.clone(); t2[1, 4:6] = 0                                   # a row without a suffix
    bad(m, t2, "empty suffix")
    t2 = t.clone(); t2[0, 6] = 0                                     # a hole in the suffix
    bad(m, t2, "contiguous run")
    t2 = t.clone(); t2[1, 5] = 0                                     # the suffix ends before the row does
    bad(m, t2, "contiguous run")
    t2 = t.clone(); t2[1, 6] = 1                                     # a one over the padding
    bad(m, t2, "contiguous run")
    t2 = t.clone(); t2[0, 1] = 1                                     # two runs
    bad(m, t2, "contiguous run")
    m2, t2 = _rows([(0, 4), (4, 2)], 8)                              # a suffix that starts at position 0
    bad(m2, t2, "position 0")
    m2 = m.clone(); m2[1, 0] = 0                                     # the mask itself is not right-padded
    bad(m2, t, "attention_mask")
    m2 = m.clone(); m2[1] = 0
    bad(m2, t, "attention_mask")
    bad(m, t[:, :7], "must match")


def _cpu_engine():
    from oracle import configs as ocfg, synth
    from pghip import configs, engine, weights
    W = synth.generate_state_dict(ocfg.TINY)
    P = weights.PackedWeights(configs.TINY, lambda k: torch.from_numpy(W[k]), device="cpu")
    return engine.PaliGemmaEngine(configs.TINY, P, device="cpu")


def test_score_refuses_bad_rows_before_any_launch():
    """score() on an engine with no device to launch on: a bad layout raises ValueError, tp > 1 NotImplementedError,
    and a good layout passes the checks and stops at the first launch, whose wrapper refuses a CPU tensor."""
    eng = _cpu_engine()
    ids = torch.full((2, 24), 5, dtype=torch.int64)
    px = torch.zeros(2, 3, 8, 8)
    mask, types = _rows([(20, 4), (18, 3)], 24)
    for m, t, what in ((mask, torch.zeros_like(types), "empty suffix"),
                       (mask, torch.ones_like(types) * mask, "position 0"),
                       (mask.flip(1), types, "attention_mask")):
        with pytest.raises(ValueError, match=what):
            eng.score(ids, px, m, t)
    with pytest.raises(RuntimeError, match="must be on the HIP device"):     # the first launch's own operand check
        eng.score(ids, px, mask, types)
    eng.tp = 2
    with pytest.raises(NotImplementedError, match="tensor parallel"):
        eng.score(ids, px, mask, types)
    with pytest.raises(ValueError, match="prefix_rows needs kv_rows"):
        eng.gemma_prefill(torch.zeros(48, 128), torch.ones(2, 24), None, 2, 24, prefix_rows=torch.ones(2))


def test_new_entry_points_reject_bad_arguments():
    """pg_attention_prefix and pg_token_logprob return hipErrorInvalidValue for null operands, empty or inconsistent
    shapes and misaligned pointers -- before any HIP call, so this runs without a device (the pointers are never
    dereferenced)."""
    from pghip import _lib, ops
    lib = _lib.load()
    p = 0x1000                                             # a non-null, 16-byte aligned, never dereferenced address

    def attn(B=2, Lq=8, Lkv=8, rows=p, prefix=p, Hq=4, Hkv=1, D=32, split_keys=0, nsplit=0, po=None, pml=None, q=p,
             o=p, k=p, vt=p, mask=None):
        return lib.pg_attention_prefix(q, Hq * D, o, Hq * D, k, 64 * D, D, D, vt, D * 64, D * 64, 64, mask, 0, 0, B,
                                       Lq, Lkv, rows, prefix, Hq, Hkv, D, 0.1, split_keys, nsplit, po, pml, 0, None,
                                       None, None)

    for kw in (dict(rows=None), dict(prefix=None), dict(q=None), dict(o=None), dict(k=None), dict(vt=None),
               dict(B=0), dict(B=-1), dict(Lq=0), dict(Lkv=0), dict(Hq=3, Hkv=2), dict(Hq=0), dict(D=36), dict(D=0),
               dict(split_keys=32, nsplit=4, po=p, pml=p),            # prefill only
               dict(nsplit=4), dict(nsplit=4, po=p), dict(nsplit=-1),  # key splits without their workspace
               dict(nsplit=9, po=p, pml=p),                           # more key splits than the merge holds
               dict(rows=p + 2), dict(prefix=p + 1), dict(q=p + 8), dict(k=p + 2), dict(vt=p + 4), dict(o=p + 2),
               dict(mask=p + 1), dict(nsplit=4, po=p + 4, pml=p)):
        assert attn(**kw) == HIP_ERROR_INVALID_VALUE, kw

    def tl(logits=p, ld=304, R=3, V=300, targets=p, logprob=p, top1=p, ws=p):
        return lib.pg_token_logprob(logits, ld, R, V, targets, logprob, top1, ws, None)

    for kw in (dict(logits=None), dict(targets=None), dict(logprob=None), dict(ws=None), dict(R=0), dict(R=-2),
               dict(V=0), dict(ld=299), dict(R=65536), dict(logits=p + 2), dict(targets=p + 4), dict(logprob=p + 1),
               dict(top1=p + 4), dict(ws=p + 8)):
        assert tl(**kw) == HIP_ERROR_INVALID_VALUE, kw
    assert ops.token_logprob_workspace(3) == 3 * (64 * 12 + 4)
    assert lib.pg_abi_version() == 13


def test_processor_batch_with_suffixes(golden):
    """batch(..., suffixes=...): every row is the pair's single-request ids, then the tokenised answer, then <eos>;
    token_type_ids is 0 over the prompt row, 1 over answer + <eos>, 0 over the padding, which engine.score_spans
    accepts; suffixes=None returns exactly the dict it returned before."""
    from transformers import AutoTokenizer
    from PIL import Image
    from processing_paligemma import PaliGemmaProcessor
    from pghip.engine import PaliGemmaEngine
    g = golden("processor")
    prompts = g["prompts"].tolist()
    rng = np.random.default_rng(7)
    imgs = [Image.fromarray(rng.integers(0, 256, (40 + 9 * j, 50, 3), dtype=np.uint8)) for j in range(len(prompts))]
    tok = AutoTokenizer.from_pretrained(os.path.join(ROOT, "tests", "golden", "tokenizer"))
    p = PaliGemmaProcessor(tok, num_image_tokens=16, image_size=56)
    answers = ["a cat", "<loc0012><loc0100> dog ; two words more", "x", "yes"]
    answers = [answers[j % len(answers)] for j in range(len(prompts))]
    single = [p(images=[im], text=[tx]) for im, tx in zip(imgs, prompts)]
    tails = [tok(a, add_special_tokens=False)["input_ids"] for a in answers]
    assert len(set(len(t) for t in tails)) > 1 and all(len(t) >= 1 for t in tails)
    out = p.batch(imgs, prompts, suffixes=answers)
    assert set(out) == {"pixel_values", "input_ids", "attention_mask", "token_type_ids"}
    B = len(prompts)
    L = max(s["input_ids"].shape[1] + len(t) + 1 for s, t in zip(single, tails))
    for k in ("input_ids", "attention_mask", "token_type_ids"):
        assert out[k].shape == (B, L), k
    for b, (s, t) in enumerate(zip(single, tails)):
        n = s["input_ids"].shape[1]
        want = s["input_ids"][0].tolist() + list(t) + [tok.eos_token_id]
        assert out["input_ids"][b, :len(want)].tolist() == want
        assert (out["input_ids"][b, len(want):] == tok.pad_token_id).all()
        assert out["attention_mask"][b].tolist() == [1] * len(want) + [0] * (L - len(want))
        assert out["token_type_ids"][b].tolist() == [0] * n + [1] * (len(t) + 1) + [0] * (L - len(want))
        assert torch.equal(out["pixel_values"][b], s["pixel_values"][0])
    prefix, lens = PaliGemmaEngine.score_spans(out["attention_mask"], out["token_type_ids"])
    assert prefix.tolist() == [s["input_ids"].shape[1] for s in single]
    assert (lens - prefix).tolist() == [len(t) + 1 for t in tails]
    # without suffixes: today's dict, key for key and bit for bit
    plain, again = p.batch(imgs, prompts), p.batch(imgs, prompts, suffixes=None)
    assert list(plain) == ["pixel_values", "input_ids", "attention_mask"] == list(again)
    Lp = max(s["input_ids"].shape[1] for s in single)
    for b, s in enumerate(single):
        n = s["input_ids"].shape[1]
        assert plain["input_ids"].shape == (B, Lp) and torch.equal(plain["input_ids"][b, :n], s["input_ids"][0])
    for k in plain:
        assert torch.equal(plain[k], again[k]) and plain[k].dtype == again[k].dtype
    with pytest.raises(ValueError):
        p.batch(imgs, prompts, suffixes=answers[:-1])
