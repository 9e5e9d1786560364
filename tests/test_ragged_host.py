"""Ragged batches (prompts of different lengths in one generate call): the checks that need no GPU.

The mask rule of engine.mask_lengths, PaliGemmaProcessor.batch on the offline tokenizer (tests/golden/tokenizer), the
argument checks of the per-row entry points (they return hipErrorInvalidValue before any HIP call, so the library
answers without a device), and the tensor-parallel refusal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1


def test_mask_lengths_accepts_right_padding_only():
    from pghip.engine import mask_lengths
    m = torch.tensor([[1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 0]])
    assert mask_lengths(m).tolist() == [4, 1, 3]
    assert mask_lengths(torch.ones(2, 5, dtype=torch.int64)).tolist() == [5, 5]
    assert mask_lengths(m.bool()).tolist() == [4, 1, 3]
    for bad, what in ((torch.tensor([[1, 1, 1], [0, 1, 1]]), "not right-padded"),          # left padding
                      (torch.tensor([[1, 1, 1, 1], [1, 0, 1, 1]]), "not right-padded"),    # a hole
                      (torch.tensor([[1, 0, 1, 0]]), "not right-padded"),
                      (torch.tensor([[1, 1], [0, 0]]), "no real token")):                  # an empty row
        with pytest.raises(ValueError, match=what):
            mask_lengths(bad)
    with pytest.raises(ValueError):
        mask_lengths(torch.ones(4))


def _cpu_engine():
    from oracle import configs as ocfg, synth
    from pghip import configs, engine, weights
    W = synth.generate_state_dict(ocfg.TINY)
    P = weights.PackedWeights(configs.TINY, lambda k: torch.from_numpy(W[k]), device="cpu")
    return engine.PaliGemmaEngine(configs.TINY, P, device="cpu")


def test_prefill_request_refuses_a_bad_mask_before_any_launch():
    """A left-padded mask, a hole and an empty row raise ValueError from prefill_request / generate on an engine that has
    no device to launch on: the check comes first."""
    eng = _cpu_engine()
    ids = torch.full((2, 20), 5, dtype=torch.int64)
    px = torch.zeros(2, 3, 8, 8)
    left = torch.ones(2, 20, dtype=torch.int64)
    left[1, :3] = 0
    hole = torch.ones(2, 20, dtype=torch.int64)
    hole[0, 18] = 0
    empty = torch.ones(2, 20, dtype=torch.int64)
    empty[1] = 0
    for mask in (left, hole, empty):
        with pytest.raises(ValueError, match="attention_mask"):
            eng.prefill_request(ids, px, mask, 4)
        with pytest.raises(ValueError, match="attention_mask"):
            eng.generate(ids, px, mask, 4)


def test_tensor_parallel_refuses_a_ragged_mask():
    """tp > 1 with a padded mask: NotImplementedError with a message that names the cause, before any launch (a CPU
    engine whose rank count is set to 2 stands in for the communicator); an all-ones mask is not refused by that check
    (it goes on to the launches, which a CPU engine cannot run)."""
    eng = _cpu_engine()
    eng.tp = 2
    ids = torch.full((2, 20), 5, dtype=torch.int64)
    mask = torch.ones(2, 20, dtype=torch.int64)
    mask[1, 19:] = 0
    with pytest.raises(NotImplementedError, match="tensor parallel"):
        eng.prefill_request(ids, torch.zeros(2, 3, 8, 8), mask, 4)
    with pytest.raises(Exception) as ei:
        eng.prefill_request(ids, torch.zeros(2, 3, 8, 8), torch.ones_like(mask), 4)
    assert not isinstance(ei.value, NotImplementedError)


def test_processor_batch_pads_right_and_keeps_each_pair(golden):
    """PaliGemmaProcessor.batch: every row is the pair's own __call__ output (ids, mask, pixels), right-padded with the
    tokenizer's pad id to the longest row; the mask is ones over the row's tokens and zeros over the padding, which
    engine.mask_lengths accepts."""
    from transformers import AutoTokenizer
    from PIL import Image
    from processing_paligemma import PaliGemmaProcessor
    from pghip.engine import mask_lengths
    g = golden("processor")
    prompts = g["prompts"].tolist()
    rng = np.random.default_rng(7)
    imgs = [Image.fromarray(rng.integers(0, 256, (40 + 9 * j, 50, 3), dtype=np.uint8)) for j in range(len(prompts))]
    tok = AutoTokenizer.from_pretrained(os.path.join(ROOT, "tests", "golden", "tokenizer"))
    p = PaliGemmaProcessor(tok, num_image_tokens=16, image_size=56)
    single = [p(images=[im], text=[tx]) for im, tx in zip(imgs, prompts)]
    lens = [s["input_ids"].shape[1] for s in single]
    assert len(set(lens)) > 1, "the fixture's prompts must differ in length for this test to see padding"
    out = p.batch(imgs, prompts)
    B, L = len(prompts), max(lens)
    assert out["input_ids"].shape == (B, L) and out["attention_mask"].shape == (B, L)
    assert out["pixel_values"].shape == (B, 3, 56, 56)
    assert out["input_ids"].dtype == single[0]["input_ids"].dtype
    for b, s in enumerate(single):
        n = lens[b]
        assert torch.equal(out["input_ids"][b, :n], s["input_ids"][0])
        assert (out["input_ids"][b, n:] == tok.pad_token_id).all()
        assert out["attention_mask"][b].tolist() == [1] * n + [0] * (L - n)
        assert torch.equal(out["pixel_values"][b], s["pixel_values"][0])
    assert mask_lengths(out["attention_mask"]).tolist() == lens
    with pytest.raises(ValueError):
        p.batch(imgs, prompts[:-1])
    with pytest.raises(ValueError):
        p.batch([], [])
    with pytest.raises(AssertionError):                     # __call__ keeps its single-pair assertion
        p(images=imgs[:2], text=prompts[:2])


def test_per_row_entry_points_reject_bad_arguments():
    """pg_attention_rows / pg_attn_decode_rows / pg_gemm_fused(PG_SLOT_ROWS) return hipErrorInvalidValue for a null
    length array, B <= 0 and inconsistent shapes -- before any HIP call, so this runs without a device (the pointers
    are never dereferenced)."""
    from pghip import _lib, ops
    lib = _lib.load()
    p = 0x1000                                             # a non-null, 16-byte aligned, never dereferenced address

    def attn(B=2, Lq=8, Lkv=8, rows=p, Hq=4, Hkv=1, D=32, split_keys=0, nsplit=0, po=None, pml=None, kcap=0, o=p):
        return lib.pg_attention_rows(p, Hq * D, o, Hq * D, p, 64 * D, D, D, p, D * 64, D * 64, 64, None, 0, 0, B, Lq,
                                     Lkv, rows, Hq, Hkv, D, 0.1, split_keys, nsplit, po, pml, kcap, None, None, None)

    assert attn(rows=None) == HIP_ERROR_INVALID_VALUE
    assert attn(B=0) == HIP_ERROR_INVALID_VALUE
    assert attn(B=-3) == HIP_ERROR_INVALID_VALUE
    assert attn(Lkv=0) == HIP_ERROR_INVALID_VALUE                    # prefill: no row can hold a key
    assert attn(Hq=3, Hkv=2) == HIP_ERROR_INVALID_VALUE
    assert attn(D=36) == HIP_ERROR_INVALID_VALUE
    assert attn(o=None) == HIP_ERROR_INVALID_VALUE
    assert attn(Lq=1, split_keys=32, nsplit=4) == HIP_ERROR_INVALID_VALUE          # split mode without a workspace
    assert attn(Lq=1, split_keys=32, nsplit=3, po=p, pml=p) == HIP_ERROR_INVALID_VALUE
    assert attn(Lq=1, split_keys=32, nsplit=4, po=p, pml=p, kcap=64) == HIP_ERROR_INVALID_VALUE   # no kd / vd

    def dec(B=2, rows=p, D=32, kcap=128, nsplit=1, nw=2, nb=2, cnt=p, Hq=4, Hkv=1):
        return lib.pg_attn_decode_rows(p, Hq * D, p, Hq * D, p, p, B, 0, rows, Hq, Hkv, D, 0.1, kcap, nsplit, nw, nb,
                                       p, p, cnt, None, None, 0, None)

    assert dec(rows=None) == HIP_ERROR_INVALID_VALUE
    assert dec(B=0) == HIP_ERROR_INVALID_VALUE
    assert dec(D=64) == HIP_ERROR_INVALID_VALUE
    assert dec(kcap=100) == HIP_ERROR_INVALID_VALUE
    assert dec(nsplit=8) == HIP_ERROR_INVALID_VALUE                  # more split waves than cache blocks
    assert dec(nb=1) == HIP_ERROR_INVALID_VALUE                      # the rounds do not cover the cache
    assert dec(cnt=None) == HIP_ERROR_INVALID_VALUE
    assert dec(Hq=4, Hkv=3) == HIP_ERROR_INVALID_VALUE

    # PG_SLOT_ROWS: needs slot_dev, and an epilogue / prologue that reads it
    fa = ops.fused_args(head_dim=32, cos_t=p, sin_t=p, pos=p, rows_per_batch=1, slot_base=-1, kc=p, vtc=p, smax=64,
                        q_heads=4, kv_heads=1)

    def gemv(fa, epi, N=192, M=2):
        return lib.pg_gemm_fused(p, 128, p, 128, None, p, N, M, N, 128, epi, 1, C.byref(fa), None)

    assert gemv(fa, ops.EPI_QKV_ROPE | ops.SLOT_ROWS) == HIP_ERROR_INVALID_VALUE           # slot_dev is null
    fa.slot_dev = p
    assert gemv(fa, ops.EPI_BF16 | ops.SLOT_ROWS) == HIP_ERROR_INVALID_VALUE               # nothing reads slot_dev
    assert gemv(fa, ops.EPI_QKV_ROPE | ops.SLOT_ROWS, N=160) == HIP_ERROR_INVALID_VALUE    # N != (Hq + 2 Hkv) * D
    assert lib.pg_gemm_fused(p, 128, p, 128, None, p, 192, 2, 192, 128, ops.EPI_QKV_ROPE | ops.SLOT_ROWS, 1, None,
                             None) == HIP_ERROR_INVALID_VALUE                              # no PgFusedArgs at all
    assert lib.pg_gemm_finalize(p, 2, p, 192, 40, 192, ops.EPI_BF16 | ops.SLOT_ROWS, None, 0, 0, C.byref(fa),
                                None) == HIP_ERROR_INVALID_VALUE
    assert lib.pg_gemm(p, 128, p, 128, None, p, 192, 2, 192, 128, ops.EPI_BF16 | ops.SLOT_ROWS, 1, None, 0, None, 0,
                       0, None) == HIP_ERROR_INVALID_VALUE
    assert lib.pg_abi_version() == 13
