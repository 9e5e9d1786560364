"""PaliGemma image->text engine on libpghip (one process per GPU).

Restates PaliGemmaForConditionalGeneration.forward (modeling_paligemma.py:257-308)
and the test_inference token loop (inference.py:45-82) as a fixed sequence of
HIP kernels:

  vision (once per request)  im2col -> patch GEMM(+bias+pos) -> 27 x [LN -> QKV GEMM(+bias, V^T)
                             -> attention -> out GEMM(split-K partials) -> LN(+partials) -> fc1 GEMM(+gelu)
                             -> fc2 GEMM(partials)] -> post-LN -> projector GEMM
  prefill                    rank scan -> embed merge -> 18 x [RMSNorm(+partials) -> QKV GEMM -> RoPE+KV write
                             -> attention -> o GEMM(partials) -> RMSNorm -> gate/up GEMM(gelu*mul) -> down GEMM
                             (partials)] -> final RMSNorm -> lm_head GEMM(+bias)
  decode step                the same per token with the GEMV kernels, split-KV attention, argmax / top-p;
                             every per-step scalar (kv length, positions, step) lives in device memory,
                             so one step is captured once as a hipGraph and replayed.  The layers run in one
                             of three routes (_decode_route), the first in two forms:
                               fin      one rank, bf16 rows.  B <= FUSE_MAX_B: o_proj and down_proj add into a
                                        fixed-point residual, norm and merge as GEMV prologues (_decode_layers_fx);
                                        FIN_MIN_B <= B <= 16: o_proj and down_proj finalise their split-K partials
                                        in-kernel, the merge is its own kernel (_decode_layers_fin);
                               fused    B <= FUSE_MAX_B otherwise (tensor parallel, USE_FIN off): RMSNorm and
                                        attention merge as GEMV prologues, fp32 slabs (_decode_layers_fused);
                               unfused  every other batch (3..4 and > 16 rows, fp8 rows, TP above FUSE_MAX_B): norm
                                        and merge as their own kernels (_decode_layers_unfused).

Output-invariant deviations from the reference: the vision
tower runs once per request instead of on every call (modeling_paligemma.py:281);
the KV cache is a static in-place buffer instead of torch.cat (modeling_gemma.py:54-55);
the generation loop computes only last-position logits.

Tensor parallelism (PackedWeights(tp_rank, tp_world) + a TPComm): every rank runs the same
kernel sequence on its head / intermediate / vocabulary slice.  The partial sums of o_proj and
down_proj are completed by one SUM all-reduce of ONE fp32 slab per sub-block (a rank's split-K
slabs are summed locally first); at prefill sizes the rows are cut into chunks and each chunk's
all-reduce runs on the communication stream while the next chunk's GEMM runs (_row_parallel).
Greedy decoding all-gathers per-rank (max, index) pairs, full logits are all-gathered by
vocabulary slice, and with at least one image per rank the SigLIP tower runs data-parallel over
the images, its features all-gathered.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Optional

import torch

from . import ops
from .tp import CaptureUnsupported, SoloComm
from .weights import PackedWeights


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def rope_tables(dim: int, n_pos: int, base: float, device):
    """cos/sin [n_pos][dim/2] exactly as GemmaRotaryEmbedding (modeling_gemma.py:112,121-135):
    inv_freq = 1/base^(arange(0,dim,2)/dim) in fp32, freqs = inv_freq * pos (fp32), cos/sin in fp32.
    Computed with torch on the CPU (the reference's own arithmetic), then uploaded."""
    inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64).float() / dim))
    pos = torch.arange(n_pos, dtype=torch.int64).float()
    freqs = inv[None, :] * pos[:, None]
    return freqs.cos().to(device).contiguous(), freqs.sin().to(device).contiguous()


def mask_lengths(attention_mask: torch.Tensor) -> torch.Tensor:
    """Per-row token counts (int64 [B], on the host) of a right-padded attention mask [B][L]: real tokens first, then
    zeros.  Raises ValueError -- on the host, before anything is launched -- for a row without a real token and for a
    zero in front of a one (left padding, a hole): generate treats row b as a request of its first len_b tokens, which
    only a right-padded mask describes."""
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask must be [B][L], got {tuple(attention_mask.shape)}")
    m = attention_mask.detach().to("cpu") != 0
    lens = m.sum(-1)
    if bool((lens == 0).any()):
        raise ValueError(f"attention_mask: row {int((lens == 0).nonzero()[0])} holds no real token")
    want = torch.arange(m.shape[1])[None, :] < lens[:, None]
    if not torch.equal(m, want):
        bad = int((m != want).any(-1).nonzero()[0])
        raise ValueError(f"attention_mask: row {bad} is not right-padded (a zero in front of a one); pad on the right "
                         "(utils.load_hf_model pins padding_side='right')")
    return lens


class KVStore:
    """Static KV cache: K [layers][B][Smax][nkv*hd] (roped), V^T [layers][B][nkv*hd][Smax], bf16, plus the
    decode-order copies kd / vd [layers][B][nkv][Smax][hd] that the QKV epilogue writes beside them and the decode
    attention kernels read (csrc/attn_common.h dec_koff / dec_voff: one contiguous KiB per load instruction)."""

    def __init__(self, layers: int, B: int, Smax: int, kv_dim: int, device, kv_heads: int = 1):
        if kv_dim % kv_heads:
            raise ValueError(f"kv_dim {kv_dim} does not split into {kv_heads} kv heads")
        self.B, self.Smax, self.kv_dim, self.kv_heads = B, Smax, kv_dim, kv_heads
        self.k = torch.zeros(layers, B, Smax, kv_dim, dtype=torch.bfloat16, device=device)
        self.vt = torch.zeros(layers, B, kv_dim, Smax, dtype=torch.bfloat16, device=device)
        self.kd = torch.zeros(layers, B * Smax * kv_dim, dtype=torch.bfloat16, device=device)
        self.vd = torch.zeros(layers, B * Smax * kv_dim, dtype=torch.bfloat16, device=device)
        self.length = 0
        self.ragged = False      # set by a prefill with per-row lengths: row b holds its own len_b < length keys

    def copy_prefix_from(self, old: "KVStore", n: int):
        """Grow: the first n positions of every layer of a smaller store (canonical and decode-order copies)."""
        nl = old.k.shape[0]
        self.k[:nl, :, :n] = old.k[:, :, :n]
        self.vt[:nl, :, :, :n] = old.vt[:, :, :, :n]
        if (old.B, old.kv_dim, old.kv_heads) != (self.B, self.kv_dim, self.kv_heads):
            raise ValueError("copy_prefix_from: the stores differ in batch or kv-head layout")
        nb = -(-n // 32) * 32                     # decode-order copies hold whole 32-key blocks per (row, kv head)
        hk, hd = self.kv_heads, self.kv_dim // self.kv_heads
        for t_new, t_old in ((self.kd, old.kd), (self.vd, old.vd)):   # [layers][B][Hkv][Smax][hd] (dec_koff / voff)
            t_new.view(-1, self.B, hk, self.Smax, hd)[:nl, :, :, :nb] = t_old.view(nl, old.B, hk, old.Smax, hd)[:, :, :, :nb]

    def repeat_rows(self, W: int) -> "KVStore":
        """A store of B * W rows whose row b * W + w is a copy of this store's row b, in all four layouts (beam search:
        every beam of a prompt starts from the prompt's cache).  Once per request, plain copies."""
        new = KVStore.__new__(KVStore)
        new.B, new.Smax, new.kv_dim, new.kv_heads = self.B * W, self.Smax, self.kv_dim, self.kv_heads
        nl = self.k.shape[0]
        new.k = self.k.repeat_interleave(W, dim=1).contiguous()
        new.vt = self.vt.repeat_interleave(W, dim=1).contiguous()
        new.kd = self.kd.view(nl, self.B, -1).repeat_interleave(W, dim=1).reshape(nl, -1).contiguous()
        new.vd = self.vd.view(nl, self.B, -1).repeat_interleave(W, dim=1).reshape(nl, -1).contiguous()
        new.length, new.ragged = self.length, self.ragged
        return new


class PaliGemmaEngine:
    DECODE_SPLIT_O = 2      # split-K of o_proj at decode (B > FUSE_MAX_B: more workgroups for the batched GEMV)
    DECODE_SPLIT_O_SMALL = 2  # ... at B <= FUSE_MAX_B: split 2 (256 workgroups, tile finalised by the second arriver).
                              # Unsplit won earlier this round (1.120-1.122 vs 1.123-1.127 ms/token); with the q|k|v
                              # weights Infinity-Cache resident split 2 wins 7 of 8 interleaved pairs, -3.7 us mean
    # 5..16 rows on the in-kernel-finalised path (F32_FIN): o_proj unsplit and down_proj split 4 (pt-448 x16: 1.391 vs
    # 1.405 ms/step at 2 / 8, profiles/r05_decode_splits_pt448x16.jsonl); PG_SPLIT_O / PG_SPLIT_DOWN override
    DECODE_SPLIT_O_FIN16, DECODE_SPLIT_DOWN_FIN16 = 1, 4
    DECODE_SPLIT_DOWN = 8   # split-K of down_proj at decode (8 vs 4: -4..6 us per pt-224 step)
    DECODE_SPLIT_KEYS = 32  # keys per wave in split-KV decode attention (one MFMA block)
    # keys per split at B <= FUSE_MAX_B: every o_proj workgroup merges all active splits in its prologue, so
    # fewer, longer splits (one wave per 32 keys, merged in LDS by attn_decode_wg_kernel) cut that re-read
    DECODE_SPLIT_KEYS_SMALL = 32
    # prefill GEMMs of at least this many rows read the row-major weight copies (weights.prefill_rowmajor)
    PREFILL_ROWMAJOR_MIN_M = 256
    # batch-1 prefill (256 <= rows <= 288, one rank, bf16): gate/up and down run as ONE row tile per 128 columns
    # (ops.TILE_M1) with this split-K -- each weight tile streams once instead of once per 256-row tile.  The q|k|v /
    # SigLIP epilogues cannot split K, so their one-tile grids would idle most CUs; o_proj runs faster on 64-row tiles
    TILE_M1_SPLIT = {"gu": 1, "down": 16}
    FUSE_MAX_B = 2          # decode batches up to this size fuse RMSNorm / attention merge into the GEMVs
    DECODE_SPLIT_TARGET = 1024  # B > FUSE_MAX_B: aim for about this many decode-attention splits (waves)
    FIN_MIN_B = 5           # FIN_MIN_B <= B <= 16: in-kernel finalisation with the merge as its own kernel
    USE_FIN = True          # single rank: the fx / fin decode layers (off: the fused form, as under tensor parallelism)
    # tensor-parallel prefill: rows per all-reduce chunk (each chunk's all-reduce overlaps the next chunk's GEMM)
    AR_CHUNK_ROWS = 4096
    # chained greedy decode (single rank): the argmax's final launch also writes the next step's input rows
    # (pg_argmax_embed), so a decode step starts at layer 0 with no embed launch (decode_state(sampler=...))
    CHAIN_EMBED = True
    # prefill linears that end a residual branch (SigLIP o / fc2, Gemma o / down) with ONE split on one rank add into
    # the residual in their epilogue (EPI_F32_RES) from this many rows on: the next norm reads the residual alone, 4 B
    # per element less than a slab write + slab read + residual rewrite; bit-identical (the same one fp32 add)
    PREFILL_RES_MIN_M = 65536
    # B > FUSE_MAX_B: split-KV attention and its merge in one launch (pg_attn_decode) from this many rounds per split
    # on; below, the split kernel + pg_attn_combine
    FUSED_MIN_ROUNDS = 2
    # B <= FUSE_MAX_B single rank, bf16: the decode GEMVs stream the lossless 13-bit weight pack (weights.frag13_pack,
    # PG_W_FRAG13) where a matrix has one -- same bits out, 18.75 % fewer weight bytes in.  W13_FORMS: the
    # launches that take it (a form that does not beat its PG_W_FRAG twin in the kernel profile leaves this list)
    W13 = os.environ.get("PG_W13", "1") != "0"
    # (measured, profiles/w13_kernel_stats_{parent,new}.csv: gate/up 22.4 -> 19.4 us, down 12.3 -> 10.8, the finalised
    # down 13.4 -> 12.8, lm_head 150.6 -> 127.4; q|k|v 4.8 -> 5.5 and o_proj 5.1 -> 5.3 lost and stay PG_W_FRAG)
    W13_FORMS = ("gu", "down", "lm")
    # ... in the 12-bit form of that pack (weights.frag12_pack, PG_W_FRAG12: 4-bit codes where a block's exponents span
    # at most 16 fields, the fifth bit plane of the others in a heap) for the launches PackedWeights holds that way
    # (PackedWeights.w12_forms = weights.W12_FORMS; a matrix is held in one form only, so the switch is PackedWeights'
    # w12 argument -- PG_W12=0 packs, and so launches, the 13-bit form throughout; W13 off turns both off)

    def __init__(self, cfg: dict, weights: PackedWeights, device="cuda", comm=None):
        self.cfg = cfg
        self.w = weights
        self.comm = comm if comm is not None else SoloComm()
        self.fp8 = bool(getattr(weights, "fp8", False))
        self.tp = getattr(weights, "tp_world", 1)
        if self.comm.world != self.tp:
            raise ValueError(f"weights packed for tp_world={self.tp}, communicator has world {self.comm.world}")
        # tuning overrides (None: unset) of the decode o_proj / down_proj split-K at every batch size (_decode_splits)
        self.split_o = self.DECODE_SPLIT_O if self.tp == 1 else 1        # smaller all-reduce messages under TP
        self.split_down = self.DECODE_SPLIT_DOWN if self.tp == 1 else max(1, self.DECODE_SPLIT_DOWN // self.tp)
        env_o, env_d = os.environ.get("PG_SPLIT_O"), os.environ.get("PG_SPLIT_DOWN")    # tuning overrides
        if env_o:
            self.split_o = int(env_o)
        if env_d:
            self.split_down = int(env_d)
        self._split_fixed = (bool(env_o), bool(env_d))  # an override holds at every batch size (_decode_splits)
        self._validate_splits()
        self.device = torch.device(device)
        self.image_token_id = cfg.get("image_token_index", 256000)
        pad = cfg.get("pad_token_id")
        self.pad_id = -1 if pad is None else pad
        self.n_img = weights.n_img
        self._rope = None
        self._rope_n = 0
        self._ws = {}
        self.graphs = {}

    # ------------------------------------------------------------------ helpers
    def _validate_splits(self):
        """Refuse split-K settings (tuning knobs included) that a kernel would reject at launch time, before any
        launch: the decode o / down GEMVs finalise in-kernel (PG_EPI_F32_FIN) with at most 8 splits."""
        w = self.w
        if not hasattr(w, "heads"):                     # vision-only pack (modeling_siglip.SiglipVisionModel)
            return
        checks = [("o_proj (PG_SPLIT_O)", self.split_o, w.heads * w.head_dim),
                  ("o_proj at batch <= 2", self.DECODE_SPLIT_O_SMALL, w.heads * w.head_dim),
                  ("down_proj (PG_SPLIT_DOWN)", self.split_down, w.inter)]
        for what, ks, K in checks:              # (a split past K's 64-wide chunks just computes a zero slab)
            if not 1 <= ks <= 8:
                raise ValueError(f"split-K {ks} for {what}: needs 1 <= split <= 8 (K = {K})")

    def _buf(self, name, shape, dtype):
        t = self._ws.get(name)
        n = math.prod(shape)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(max(n, 1), dtype=dtype, device=self.device)
            self._ws[name] = t
        return t[:n].view(*shape)

    def rope(self, n_pos: int):
        if self._rope is None or self._rope_n < n_pos:
            n = _rup(max(n_pos, 1024), 1024)
            self._rope = rope_tables(self.w.head_dim, n, self.w.rope_theta, self.device)
            self._rope_n = n
        return self._rope

    def new_cache(self, B: int, Smax: int) -> KVStore:
        w = self.w
        return KVStore(w.t_layers, B, _rup(Smax, 64), w.kv_heads * w.head_dim, self.device, kv_heads=w.kv_heads)

    # ------------------------------------------------------------------ vision tower
    def vision(self, pixel_values: torch.Tensor, want_hidden: bool = False, taps: Optional[list] = None,
               _split_batch: Optional[int] = None):
        """SiglipVisionModel.forward + projector (modeling_siglip.py:312-334, modeling_paligemma.py:60-65).
        Returns image features fp32 [B*N][P] (projector output, unscaled) and optionally the
        post-LN vision output fp32 [B*N][hv].  _split_batch (the data-parallel call of a rank's slice): choose the
        split-K and attention key splits as for a batch of that many images, so that each image's features are
        bit-identical to the single-rank run over the whole batch."""
        w = self.w
        px = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        B = px.shape[0]
        if (_split_batch is None and self.tp > 1 and B >= self.tp and B % self.tp == 0
                and not want_hidden and taps is None and w.proj_w is not None):
            # data-parallel over the images (output-invariant): this rank encodes its B/W images,
            # then the projected features [B*N][P] are all-gathered in rank order = image order.  The rank-local
            # call takes the whole batch's split choices, so the features equal the replicated run's bit for bit
            Bl = B // self.tp
            mine = self.vision(px[self.comm.rank * Bl:(self.comm.rank + 1) * Bl], _split_batch=B)
            feats = torch.empty(B * w.n_img, w.proj_dim, dtype=torch.float32, device=self.device)
            self.comm.all_gather(feats, mine)
            return feats
        N, hv, nh, hd = w.n_img, w.v_hidden, w.v_heads, w.v_head_dim
        M = B * N
        patches = self._buf("v_patches", (M, w.patch_k), torch.bfloat16)
        ops.patch_im2col(px, w.patch, patches)
        resid = self._buf("v_resid", (M, hv), torch.float32)
        ops.gemm(patches, w.patch_w, resid, epi=ops.EPI_F32_POS, bias=w.patch_b, aux=w.pos_emb, aux_rows=N)
        if taps is not None:
            taps.append(resid.clone())
        xn = self._buf("v_xn", (M, hv), torch.bfloat16)
        qkv = self._buf("v_qkv", (M, 3 * hv), torch.bfloat16)
        vt = self._buf("v_vt", (hv, M + 32), torch.bfloat16)            # rows padded: attention reads 32-key blocks
        attn = self._buf("v_attn", (M, hv), torch.bfloat16)
        h = self._buf("v_h", (M, w.v_inter), torch.bfloat16)
        Bs = _split_batch or B                                            # the batch the splits are chosen for
        s_o = ops.gemm_ksplit(Bs * N, hv, hv)
        s_2 = ops.gemm_ksplit(Bs * N, hv, w.v_inter)
        ks_v = self._key_split_args("v", Bs, N, N, nh, nh, hd)
        part = self._buf("v_part", (max(s_o, s_2), M, hv), torch.float32)
        res = M >= max(17, self.PREFILL_RES_MIN_M)       # one-split o / fc2 add into the residual (EPI_F32_RES)
        res_o, res_2 = res and s_o == 1, res and s_2 == 1
        ns = 0
        for L in w.vl:
            ops.norm_residual(resid, L["ln1_w"], b=L["ln1_b"], mode=ops.NORM_LAYER, eps=w.v_eps, partials=part,
                              nsplit=ns, out=xn, write_resid=ns > 0)
            ops.gemm(xn, L["qkv_w"], qkv, epi=ops.EPI_BF16_VT, bias=L["qkv_b"], aux_out=vt, aux_ld=M + 32,
                     aux_n=2 * hv, split_m=Bs * N)
            ops.attention(qkv, 3 * hv, attn, hv, qkv[:, hv:], N * 3 * hv, hd, 3 * hv, vt, N, hd * (M + 32), M + 32,
                          B=B, Lq=N, Lkv=N, Hq=nh, Hkv=nh, D=hd, scale=1.0 / (hd ** 0.5), **ks_v)
            if res_o:
                ops.gemm(attn, L["o_w"], resid, epi=ops.EPI_F32_RES, bias=L["o_b"])
            else:
                ops.gemm(attn, L["o_w"], part, epi=ops.EPI_F32, bias=L["o_b"], ksplit=s_o)
            ops.norm_residual(resid, L["ln2_w"], b=L["ln2_b"], mode=ops.NORM_LAYER, eps=w.v_eps, partials=part,
                              nsplit=0 if res_o else s_o, out=xn, write_resid=not res_o)
            ops.gemm(xn, L["fc1_w"], h, epi=ops.EPI_BF16_GELU, bias=L["fc1_b"], split_m=Bs * N)
            if res_2:
                ops.gemm(h, L["fc2_w"], resid, epi=ops.EPI_F32_RES, bias=L["fc2_b"])
                ns = 0
            else:
                ops.gemm(h, L["fc2_w"], part, epi=ops.EPI_F32, bias=L["fc2_b"], ksplit=s_2)
                ns = s_2
            if taps is not None:                                          # debug: residual after the layer
                taps.append((resid + part[:ns].sum(0)).clone())
        hid = torch.empty(M, hv, dtype=torch.float32, device=self.device) if want_hidden else None
        ops.norm_residual(resid, w.post_w, b=w.post_b, mode=ops.NORM_LAYER, eps=w.v_eps, partials=part, nsplit=ns,
                          out=xn, out_f32=hid)
        feats = torch.empty(M, max(w.proj_dim, 1), dtype=torch.float32, device=self.device)
        if w.proj_w is None:                                              # vision-only pack
            return (None, hid) if want_hidden else None
        ops.gemm(xn, w.proj_w, feats, epi=ops.EPI_F32)
        return (feats, hid) if want_hidden else feats

    # ------------------------------------------------------------------ Gemma stack (prefill, T = B*L rows)
    def _embed_kw(self) -> dict:
        """The constants every embedding launch takes (pg_embed_merge, pg_argmax_embed): the image and pad ids, the
        image features' 1/sqrt(P) and the text rows' sqrt(H)."""
        return dict(image_id=self.image_token_id, pad_id=self.pad_id, img_scale=float(self.w.proj_dim ** -0.5),
                    normalizer=float(self.w.hidden ** 0.5))

    def embed_merge(self, input_ids: torch.Tensor, feats: torch.Tensor, out: torch.Tensor, rank=None):
        ids = input_ids.reshape(-1)
        n = ids.numel()
        if rank is None and n > 64:
            rank = self._buf("rank", (n,), torch.int32)
            ops.image_rank(ids, self.image_token_id, rank)
        ops.embed_merge(ids, rank, self.w.embed, feats, feats.shape[0] if feats is not None else 0, out,
                        **self._embed_kw())

    def gemma_prefill(self, x_resid: torch.Tensor, positions: torch.Tensor, cache: KVStore, B: int, L: int,
                      logits_rows: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                      want_hidden: bool = False, want_logits: bool = True, taps: Optional[list] = None,
                      kv_rows: Optional[torch.Tensor] = None, prefix_rows: Optional[torch.Tensor] = None,
                      return_rows: bool = False):
        """GemmaForCausalLM.forward after the *sqrt(H) (modeling_gemma.py:510-534) on resid fp32 [B*L][H]
        (already scaled).  Fills cache slots [0, L).  logits_rows: int32 rows to emit logits for (None = all).
        kv_rows (int32 [B] on the device; a right-padded batch): row b's queries attend its first kv_rows[b] keys
        only (ops.attention_rows); the padding's own rows compute finite values nobody reads.
        prefix_rows (int32 [B] on the device, with kv_rows): row b is a prefix-LM sequence -- its first prefix_rows[b]
        positions attend one another, the later ones causally (ops.attention_prefix; score()).
        return_rows: also return the final norm's bf16 rows [rows][H] (the lm_head's input), as a third value."""
        if kv_rows is not None and mask is not None:
            raise ValueError("gemma_prefill: per-row key counts replace the additive mask, pass one of them")
        if prefix_rows is not None and (kv_rows is None or mask is not None):
            raise ValueError("gemma_prefill: prefix_rows needs kv_rows (each row's length) and excludes the additive mask")
        w = self.w
        T = B * L
        H, I, nh, nkv, hd = w.hidden, w.inter, w.heads, w.kv_heads, w.head_dim
        cos_t, sin_t = self.rope(L + 2)
        xn = self._buf("t_xn", (T, H), torch.bfloat16)
        qb = self._buf("t_q", (T, nh * hd), torch.bfloat16)
        attn = self._buf("t_attn", (T, nh * hd), torch.bfloat16)
        h = self._buf("t_h", (T, I), torch.bfloat16)
        s_o = self._ksplit(T, H, nh * hd) if T > 16 else self.DECODE_SPLIT_O
        s_d = self._ksplit(T, H, I) if T > 16 else self.DECODE_SPLIT_DOWN
        part = self._buf("t_part", (max(s_o, s_d), T, H), torch.float32)
        pos = positions.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        ks_t = self._key_split_args("t", B, L, L, nh, nkv, hd) if mask is None else {}
        ns = 0
        if taps is not None:
            taps.append(x_resid.clone())
        kvd = nkv * hd
        for i, Lw in enumerate(w.tl):
            xin = self._norm(x_resid, Lw["in_w"], part, ns, xn, T)
            # q|k|v projection + RoPE + KV-cache append in one GEMM (modeling_gemma.py:274-302)
            fa = ops.fused_args(head_dim=hd, cos_t=cos_t, sin_t=sin_t, pos=pos, rows_per_batch=L, slot_base=0,
                                kc=cache.k[i], vtc=cache.vt[i], smax=cache.Smax, q_heads=nh, kv_heads=nkv,
                                kd=cache.kd[i], vd=cache.vd[i])
            self._lin(xin, Lw, "qkv", qb, ops.EPI_QKV_ROPE, T, fa=fa)
            a_args = (qb, nh * hd, attn, attn.stride(0), cache.k[i], cache.Smax * kvd, hd, kvd,
                      cache.vt[i], kvd * cache.Smax, hd * cache.Smax, cache.Smax)
            if prefix_rows is not None:
                ops.attention_prefix(*a_args, B=B, Lq=L, Lkv=L, lkv_rows=kv_rows, prefix_rows=prefix_rows, Hq=nh,
                                     Hkv=nkv, D=hd, scale=1.0 / math.sqrt(hd), **ks_t)
            elif kv_rows is not None:
                ops.attention_rows(*a_args, B=B, Lq=L, Lkv=L, lkv_rows=kv_rows, Hq=nh, Hkv=nkv, D=hd,
                                   scale=1.0 / math.sqrt(hd), **ks_t)
            else:
                ops.attention(*a_args, B=B, Lq=L, Lkv=L, Hq=nh, Hkv=nkv, D=hd, scale=1.0 / math.sqrt(hd),
                              mask=mask, mask_bs=(mask.stride(0) if mask is not None else 0),
                              mask_rs=(mask.stride(-2) if mask is not None else 0), **ks_t)
            n_o = self._row_parallel(attn, Lw, "o", part, T, s_o, resid=x_resid)
            xin = self._norm(x_resid, Lw["post_w"], part, n_o, xn, T)
            if self._mx_prefill(T):
                # MX h: e4m3 rows + block scales from the gate/up epilogue, straight into the down GEMM
                h8 = self._buf("t_h8", (T, I), torch.uint8)
                hs = self._buf("t_hs", (T, I // 32), torch.uint8)
                x8, xs = xin
                ops.gemm8(x8, xs, Lw["gu_w8"], Lw["gu_s8"], h8, epi=ops.EPI_BF16_GELU_MUL, M=T, mx_out=hs)
                ns = self._row_parallel(("mx", h8, hs), Lw, "down", part, T, s_d, resid=x_resid)
            else:
                self._lin(xin, Lw, "gu", h, ops.EPI_BF16_GELU_MUL, T)
                ns = self._row_parallel(h, Lw, "down", part, T, s_d, resid=x_resid)
            if taps is not None:
                taps.append((x_resid + part[:ns].sum(0)).clone())
        cache.length = L
        cache.ragged = kv_rows is not None
        rows = logits_rows.numel() if logits_rows is not None else T
        xf = self._buf("t_xf", (rows, H), torch.bfloat16)
        hid = torch.empty(rows, H, dtype=torch.float32, device=self.device) if want_hidden else None
        ops.norm_residual(x_resid, w.final_w, mode=ops.NORM_RMS, partials=part, nsplit=ns, out=xf, out_f32=hid,
                          row_map=logits_rows, write_resid=False)
        logits = self.lm_head(xf, rows, fresh=True) if want_logits else None
        return (logits, hid, xf) if return_rows else (logits, hid)

    def _key_split_args(self, tag: str, B: int, Lq: int, Lkv: int, Hq: int, Hkv: int, D: int) -> dict:
        """pg_attention keyword arguments for a key-split prefill attention (ops.prefill_key_splits; {} = unsplit):
        the split count and its (O, m, l) workspace."""
        nks = ops.prefill_key_splits(B, Lq, Lkv, Hq, Hkv)
        if nks <= 1:
            return {}
        no, nml = ops.prefill_split_workspace(B, Lq, Hq, Hkv, D, nks)
        return dict(nsplit=nks, part_o=self._buf(f"pf_po_{tag}", (no,), torch.float32),
                    part_ml=self._buf(f"pf_pml_{tag}", (nml,), torch.float32))

    def _fp8_rows(self, M: int) -> bool:
        return self.fp8 and M > 16

    def _mx_prefill(self, M: int) -> bool:
        """The fp8 prefill MLP on MX h: the tile GEMMs (more than 32 rows) with row-major fp8 weights.  The 128 x 128
        fp8 gate/up tile writes h as e4m3 with one E8M0 scale per 32 columns (PgFusedArgs.mx_out) and the fp8 down GEMM
        stages those block scales beside h (mx_in) -- no row quantiser launch between them."""
        L0 = self.w.tl[0]
        # (under TP the down projection may run as row chunks (_row_parallel): each must keep > 32 rows)
        chunks_ok = self.tp == 1 or M < 2 * self.AR_CHUNK_ROWS or self.AR_CHUNK_ROWS >= 64
        return (self._fp8_rows(M) and M > 32 and "gu_w8" in L0 and "down_w8" in L0 and self.w.inter % 128 == 0
                and chunks_ok)

    def _mx_decode(self, B: int) -> tuple:
        """(MX h, MX norms) for a B-row decode step: the 17..32-row fp8 GEMV path with the packed fp8 weights.
        MX h: the gate/up epilogue writes h as e4m3 with one E8M0 scale per 32 columns (mx_out) and the down GEMV reads
        those block scales into its MFMAs (mx_in) -- no quantiser launch and no cross-workgroup row maximum.  MX norms:
        the RMSNorms in front of the q|k|v, gate/up and lm_head GEMVs write MX rows of x*(1+w) with per-1024-column sums
        of squares (pg_norm_residual_mx) and the GEMV applies rstd to its outputs -- no norm + row quantiser pair."""
        w = self.w
        L0 = w.tl[0]
        mx_h = (self._fp8_rows(B) and B <= 32 and "gu_w8f" in L0 and "down_w8f" in L0 and w.inter % 128 == 0
                and w.hidden <= 4096)
        mx_n = mx_h and "qkv_w8f" in L0 and w.hidden % 1024 == 0 and getattr(w, "lm_w8f", None) is not None
        return mx_h, mx_n

    def _ksplit(self, M: int, N: int, K: int) -> int:
        """split-K of an fp32-partial GEMM (fp8 operands: the kernels count K in byte pairs).  A GEMM that will
        run as row blocks (_lin16 / _row_head) takes the split that suits its whole-tile head: the pt-448 x16
        down projection then runs 512 full-K tiles in 2 rounds instead of 1536 third-K tiles in 6, and two
        fewer fp32 slabs are written and re-read by the next RMSNorm."""
        if self._fp8_rows(M):
            return ops.gemm_ksplit(M, N, K // 2)
        m1 = self._tile_m1(M, "down" if K == self.w.inter else "o")
        if m1:
            return m1
        Mh = M // 256 * 256
        if 0 < Mh < M:
            s = ops.gemm_ksplit(Mh, N, K)
            if self._row_head(M, N, s):
                return s
        return ops.gemm_ksplit(M, N, K)

    def _tile_m1(self, M: int, name: str) -> int:
        """split-K of a batch-1 prefill linear run as one row tile (ops.TILE_M1), 0 when it does not apply."""
        if self.fp8 or self.tp != 1 or not 256 <= M <= 288 or M < self.PREFILL_ROWMAJOR_MIN_M:
            return 0
        ks = self.TILE_M1_SPLIT.get(name, 0)
        K = self.w.inter if name == "down" else self.w.hidden
        return ks if ks * 64 <= K else 0

    def _lin(self, x, Lw: dict, name: str, out: torch.Tensor, epi: int, M: int, ksplit: int = 1, fa=None):
        """One Gemma linear on M rows: fp8 (_lin8) when x comes as fp8 rows or the weights are fp8 and M > 16, else
        bf16 (_lin16)."""
        lin = self._lin8 if isinstance(x, tuple) or self._fp8_rows(M) else self._lin16
        return lin(x, Lw, name, out, epi, M, ksplit, fa)

    def _lin8(self, x, Lw: dict, name: str, out: torch.Tensor, epi: int, M: int, ksplit: int, fa):
        """An fp8 Gemma linear (PG_FP8, per-channel weight scales).  x: ("mx", e4m3 rows, [M][K/32] block scales) for
        the tile GEMM on MX rows; (e4m3 rows, row scales) from _norm or the attention kernel; or bf16 rows, quantised
        here (pg_quant_fp8).  Up to 32 rows stream the fragment-packed weights (the fp8 GEMV) where the pack has them."""
        if isinstance(x, tuple) and x[0] == "mx":
            return ops.gemm8(x[1], None, Lw[name + "_w8"], Lw[name + "_s8"], out, epi=epi, M=M, ksplit=ksplit, fa=fa,
                             mx_in=x[2])
        if not isinstance(x, tuple):
            x8, xs = self._x8(M, x.shape[1])
            ops.quant_fp8(x, x8, xs, M=M)
        else:
            x8, xs = x
        if M <= 32 and name + "_w8f" in Lw:
            return ops.gemm8(x8, xs, Lw[name + "_w8f"], Lw[name + "_s8"], out, epi=epi, M=M, ksplit=ksplit, fa=fa,
                             frag=True)
        return ops.gemm8(x8, xs, Lw[name + "_w8"], Lw[name + "_s8"], out, epi=epi, M=M, ksplit=ksplit, fa=fa)

    def _lin16(self, x: torch.Tensor, Lw: dict, name: str, out: torch.Tensor, epi: int, M: int, ksplit: int, fa):
        """A bf16 Gemma linear: fragment-packed W, or from PREFILL_ROWMAJOR_MIN_M rows on the row-major copy -- as one
        row tile (_tile_m1), as row blocks (_row_head: fp32 slabs, and gate/up), or as one launch."""
        W, flag = Lw[name + "_w"], self.w.wflag
        if M >= self.PREFILL_ROWMAJOR_MIN_M and name + "_wr" in Lw:
            W, flag = Lw[name + "_wr"], 0
            if fa is None and self._tile_m1(M, name) == ksplit:
                return ops.gemm(x, W, out, epi=epi | ops.TILE_M1, ksplit=ksplit)
        if fa is not None:
            return ops.gemm_fused(x, W, out, fa, epi=epi | flag, M=M)
        if epi == ops.EPI_F32:
            Mh = self._row_head(M, W.shape[0], ksplit)
            if Mh:
                return self._lin_row_blocks(x, W, out, epi | flag, M, Mh, ksplit)
        if epi == ops.EPI_BF16_GELU_MUL:
            Mh = self._row_head(M, W.shape[0], 1)
            if Mh:      # gate/up at pt-448 x16: 8192 whole tiles (32 rounds) + a 128-row tail, not 33 rounds
                ops.gemm(x[:Mh], W, out[:Mh], epi=epi | flag)
                return ops.gemm(x[Mh:M], W, out[Mh:M], epi=epi | flag)
        return ops.gemm(x, W, out, epi=epi | flag, ksplit=ksplit)

    def _lin_row_blocks(self, x: torch.Tensor, W: torch.Tensor, out: torch.Tensor, epi: int, M: int, Mh: int,
                        ksplit: int):
        """A bf16 fp32-slab GEMM as a head of Mh rows (_row_head) and a tail: the 256-row tiles of the first Mh rows
        fill whole rounds of CUs; the ragged last rows (pt-448 x16: 128 of 16512) run as a small GEMM instead of one
        more mostly idle round.  Both write the same [ksplit][M][N] slabs (PgFusedArgs.slab_rows)."""
        fr = ops.fused_args(slab_rows=M)
        ops.gemm_fused(x[:Mh], W, out, fr, epi=epi, M=Mh, ksplit=ksplit, ldc=out.stride(-2))
        N, K, Mt = W.shape[0], W.shape[1], M - Mh
        st = max(ksplit, ops.split_for(math.ceil(Mt / 64) * math.ceil(N / 128), K // 64, max_split=8))
        if st > ksplit:
            # the tail's own deeper split (its 64x128 tiles alone leave most CUs idle), summed into
            # slab 0's tail rows; the other slabs' tail rows are zeroed (the head never writes them)
            tp = self._buf("row_tail", (st, Mt, N), torch.float32)
            ops.gemm(x[Mh:M], W, tp, epi=epi, ksplit=st)
            ops.slab_sum(tp, out[0, Mh:M])
            if ksplit > 1:
                out[1:ksplit, Mh:M].zero_()
            return out
        tail = out.view(-1)[Mh * out.stride(-2):]
        return ops.gemm_fused(x[Mh:M], W, tail, fr, epi=epi, M=Mt, ksplit=ksplit, ldc=out.stride(-2))

    def _x8(self, M: int, K: int) -> tuple:
        """The (e4m3 rows [M][K], fp32 row scales [M]) buffers of an fp8 linear's K-wide input."""
        return self._buf(f"x8_{K}", (M, K), torch.uint8), self._buf(f"xs_{K}", (M,), torch.float32)

    @staticmethod
    def _row_head(M: int, N: int, ksplit: int, cus: int = ops.CUS) -> int:
        """Rows of an fp32-slab prefill GEMM to issue as whole 256-row tiles, 0 to keep it one launch: only
        in the one-tile-per-CU regime (>= `cus` 256x256 tiles) and when dropping the ragged last row tile
        saves a round of CUs (Gemma o / down at pt-448 x16: 2.03 -> 2 and 6.1 -> 6 rounds)."""
        Mh = M // 256 * 256
        tn = (N + 255) // 256
        if Mh == M or Mh == 0 or (M + 255) // 256 * tn * ksplit < cus:
            return 0
        rounds = lambda tiles: (tiles + cus - 1) // cus  # noqa: E731
        return Mh if rounds(Mh // 256 * tn * ksplit) < rounds((M + 255) // 256 * tn * ksplit) else 0

    def _norm(self, resid: torch.Tensor, norm_w: torch.Tensor, part, nsplit: int, xn: torch.Tensor, M: int):
        """Gemma RMSNorm of the residual (+ split-K partials) feeding a linear: bf16 rows, or fp8 rows with
        their scales (one launch, pg_norm_residual_fp8) when that linear runs on the fp8 path."""
        if self._fp8_rows(M):
            x8, xs = self._x8(M, resid.shape[-1])
            return ops.norm_residual_fp8(resid, norm_w, x8, xs, mode=ops.NORM_RMS, partials=part, nsplit=nsplit,
                                         write_resid=nsplit > 0)
        ops.norm_residual(resid, norm_w, mode=ops.NORM_RMS, partials=part, nsplit=nsplit, out=xn,
                          write_resid=nsplit > 0)
        return xn

    def _allreduce_slabs(self, part: torch.Tensor, ns: int) -> int:
        """Complete a row-parallel linear's partial sums: one rank keeps its ns split-K slabs (the next norm adds
        them); under TP the rank's slabs are summed into slab 0 on the way into ONE all-reduce of [rows][H] fp32
        (xGMI: inside the exchange kernel; RCCL / gloo: a slab-sum launch first).  Returns the slab count the
        next norm must add."""
        if self.tp == 1:
            return ns
        return self.comm.all_reduce_slabs(part[:ns], ns)

    def _row_parallel(self, x: torch.Tensor, Lw: dict, name: str, part: torch.Tensor, T: int, ks: int,
                      resid: Optional[torch.Tensor] = None) -> int:
        """A row-parallel prefill linear (o_proj / down_proj) into fp32 partial slabs; returns how many slabs the
        next norm must add.  One rank: `ks` split-K slabs.  Tensor parallel: ONE slab, completed by a SUM all-reduce
        -- a rank's split-K slabs are summed locally first (slab_sum), so every sub-block moves T*H*4 bytes instead
        of ks times that.  From 2 * AR_CHUNK_ROWS rows on, the rows run as chunks with one split each: chunk c's
        all-reduce is issued asynchronously (comm stream) and overlaps chunk c+1's GEMM."""
        if self.tp == 1:
            # (not where the bf16 GEMM runs as row blocks: its ragged tail takes a deeper split of its own, which a
            # one-split epilogue cannot -- pt-448 x16 prefill 82.9 -> 86.6 ms with it)
            row_blocks = not self._fp8_rows(T) and self._row_head(T, self.w.hidden, 1) > 0
            if resid is not None and ks == 1 and T >= max(17, self.PREFILL_RES_MIN_M) and not row_blocks:
                self._lin(x, Lw, name, resid, ops.EPI_F32_RES, T)     # the residual add in the epilogue
                return 0
            self._lin(x, Lw, name, part, ops.EPI_F32, T, ksplit=ks)
            return ks
        # at most AR_CHUNK_ROWS rows per chunk (4096 x 2048 fp32 = the xGMI exchange's 2^23 cap: no chunk spills to
        # the process group)
        C = -(-T // self.AR_CHUNK_ROWS) if T >= 2 * self.AR_CHUNK_ROWS else 1
        if C <= 1:
            self._lin(x, Lw, name, part, ops.EPI_F32, T, ksplit=ks)
            return self.comm.all_reduce_slabs(part[:ks], ks)
        bounds = [T * c // C for c in range(C + 1)]
        works = []
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            xc = ("mx", x[1][r0:r1], x[2][r0:r1]) if isinstance(x, tuple) else x[r0:r1]
            self._lin(xc, Lw, name, part[0, r0:r1], ops.EPI_F32, r1 - r0, ksplit=1)
            works.append(self.comm.all_reduce_async(part[0, r0:r1]))
        for wk in works:
            wk.wait()
        return 1

    def lm_head(self, xf: torch.Tensor, rows: int, fresh: bool = False, name: str = "lm"):
        """Full-vocabulary logits fp32 [rows][V] from normalised bf16 rows (modeling_gemma.py:530-534).
        Under TP each rank computes its vocabulary slice and an all-gather assembles the rows (each slice
        crosses the links once; the zero-padded SUM of round 2 moved W times the bytes)."""
        w = self.w
        alloc = (lambda shape: torch.empty(*shape, dtype=torch.float32, device=self.device)) if fresh else \
            (lambda shape: self._buf(name, shape, torch.float32))
        if self.tp == 1:
            logits = alloc((rows, w.vocab_local_pad))      # lm_w rows padded to 16 (fragment packing)
            self._lm_gemm(xf, rows, logits)
            return logits[:, :w.vocab]
        vl, vlp = w.vocab_local, w.vocab_local_pad
        loc = self._buf(name + "_loc", (rows, vlp), torch.float32)
        self._lm_gemm(xf, rows, loc)
        g = self._buf(name + "_gather", (self.tp, rows, vlp), torch.float32)
        self.comm.all_gather(g, loc)                                      # [rank][rows][vocab slice]
        out = alloc((rows, w.vocab))
        out.view(rows, self.tp, vl).copy_(g[:, :, :vl].permute(1, 0, 2))
        return out

    def _lm_gemm(self, xf: torch.Tensor, rows: int, out: torch.Tensor):
        """This rank's lm_head rows [rows][vocab_local_pad] fp32 (+ bias) from normalised bf16 rows: bf16 GEMV / GEMM,
        or with fp8 weights at 17..32 rows the e4m3 rows through the fp8 GEMV (half the 1.05 GB of bf16 weights)."""
        w = self.w
        if isinstance(xf, tuple):                   # ("mx", e4m3 rows, block scales, sums of squares)
            _, x8, xs, ss = xf
            return ops.gemm8(x8, None, w.lm_w8f, w.lm_s8, out, epi=ops.EPI_F32, M=rows, bias=w.lm_bias, frag=True,
                             mx_in=xs, ss_in=ss)
        if self._fp8_rows(rows) and rows <= 32 and getattr(w, "lm_w8f", None) is not None:
            x8, xs = self._x8(rows, xf.shape[1])
            ops.quant_fp8(xf, x8, xs, M=rows)
            return ops.gemm8(x8, xs, w.lm_w8f, w.lm_s8, out, epi=ops.EPI_F32, M=rows, bias=w.lm_bias, frag=True)
        return ops.gemm(xf, w.lm_w, out, epi=ops.EPI_F32 | w.wflag, bias=w.lm_bias)

    # ------------------------------------------------------------------ decode step (graph-capturable)
    def _chain_ok(self, sampler) -> bool:
        return (self.CHAIN_EMBED and self.tp == 1 and sampler is not None and not sampler.get("do_sample")
                and sampler.get("beam") is None)      # a beam step re-embeds st["ids"]: its rows change hypothesis

    def decode_state(self, B: int, cache: KVStore, positions_next: torch.Tensor, max_steps: int, sampler=None):
        """Device-resident decode state: ids, positions, kv length, step counter, token history.

        With the loop's sampler given (generate / bench) and greedy single-rank decoding, the state is
        *chained*: every sample() also writes the embedding of the sampled ids into the decode input buffer,
        and decode_step skips its embed launch.  A caller that writes st["ids"] itself (teacher forcing)
        builds the state without a sampler."""
        st = {
            "ids": torch.zeros(B, dtype=torch.int64, device=self.device),
            "pos": positions_next.to(device=self.device, dtype=torch.int32).reshape(B).contiguous().clone(),
            "kv_len": torch.full((1,), cache.length, dtype=torch.int32, device=self.device),
            "step": torch.zeros(1, dtype=torch.int32, device=self.device),
            "hist": torch.zeros(max_steps + 1, B, dtype=torch.int64, device=self.device),
            "ws": torch.empty(B * 64 * 2, dtype=torch.float32, device=self.device),
            "chain": self._chain_ok(sampler),
            # per-row kv lengths (a prefill with a right-padded mask): pos[b] - 1 is row b's kv length before its
            # token and the slot it appends at, so the step reads st["pos"] where it read st["kv_len"]
            "ragged": bool(getattr(cache, "ragged", False)),
        }
        return st

    def _decode_route(self, B: int) -> str:
        """The route the layers of a B-row decode step take: "fin" (_decode_layers_fx at B <= FUSE_MAX_B,
        _decode_layers_fin above), "fused" (_decode_layers_fused) or "unfused" (_decode_layers_unfused)."""
        fin_rows = B <= self.FUSE_MAX_B or self.FIN_MIN_B <= B <= 16
        if self.tp == 1 and self.USE_FIN and fin_rows and not self._fp8_rows(B):
            return "fin"
        return "unfused" if B > self.FUSE_MAX_B else "fused"

    def _decode_splits(self, B: int, route: str) -> tuple:
        """(o_proj, down_proj) split-K of a B-row decode step on `route`.  A PG_SPLIT_O / PG_SPLIT_DOWN override holds
        everywhere; else 5..16 rows finalised in-kernel take the *_FIN16 pair, B <= FUSE_MAX_B on one rank takes
        DECODE_SPLIT_O_SMALL, and everything else split_o / split_down."""
        so, sd = self.split_o, self.split_down
        fixed_o, fixed_d = self._split_fixed
        if route == "fin" and B > self.FUSE_MAX_B:
            so = so if fixed_o else self.DECODE_SPLIT_O_FIN16
            sd = sd if fixed_d else self.DECODE_SPLIT_DOWN_FIN16
        elif self.tp == 1 and B <= self.FUSE_MAX_B and not fixed_o:
            so = self.DECODE_SPLIT_O_SMALL
        return so, sd

    def _decode_ws(self, B: int, cache: KVStore) -> SimpleNamespace:
        """What a B-row decode step over `cache` fixes before its first launch: the layer form and its split-K pair,
        the split-KV geometry (SK keys per split, nsplit splits, dt = head_dim padded to 16), the RoPE tables and the
        buffers -- the residual pair res_a / res_b, normalised rows xn, q rows qb, MLP rows h, the o / down split-K
        slabs part (as many as the route's deeper split writes) and the attention partials part_o / part_ml."""
        w = self.w
        H, nh, nkv, hd = w.hidden, w.heads, w.kv_heads, w.head_dim
        route = self._decode_route(B)
        so, sd = self._decode_splits(B, route)
        cos_t, sin_t = self.rope(cache.Smax + 2)
        SK = self._split_keys(B, cache.Smax)
        nsplit = _rup((cache.Smax + SK - 1) // SK, 4)
        dt = (hd + 15) // 16 * 16
        ns_ws = max(nsplit, ops.decode_plan(B, nkv, cache.Smax)[0]) if B > self.FUSE_MAX_B else nsplit
        return SimpleNamespace(
            B=B, route=route, so=so, sd=sd, SK=SK, nsplit=nsplit, dt=dt, cos_t=cos_t, sin_t=sin_t,
            ragged=False, sr=0,         # per-row kv lengths (decode_step sets them from the state)
            res_a=self._buf("d_res_a", (B, H), torch.float32),
            res_b=self._buf("d_res_b", (B, H), torch.float32),
            xn=self._buf("d_xn", (B, H), torch.bfloat16),
            qb=self._buf("d_q", (B, nh * hd), torch.bfloat16),
            h=self._buf("d_h", (B, w.inter), torch.bfloat16),
            part=self._buf("d_part", (max(so, sd), B, H), torch.float32),
            part_o=self._buf("d_po", (B * nkv * ns_ws * 16 * dt,), torch.float32),
            part_ml=self._buf("d_pml", (B * nkv * ns_ws * 16 * 2,), torch.float32))

    def decode_step(self, st: dict, cache: KVStore, feats: Optional[torch.Tensor], sampler: dict):
        """One token for B rows: embed(ids) -> 18 layers -> lm_head -> argmax/top-p (advances the state).  The layers
        run in the form _decode_route picks for B, on the buffers and splits of one _decode_ws record.  Returns the
        step's logits; with a grammar in the sampler they are the masked ones (-inf where a row's DFA state did not
        allow the token: sample() masks the buffer in place)."""
        w = self.w
        B = st["ids"].numel()
        ws = self._decode_ws(B, cache)
        ws.ragged = bool(st.get("ragged"))
        ws.sr = ops.SLOT_ROWS if ws.ragged else 0   # OR-ed into the epi of the launches that read slot_dev
        chain = bool(st.get("chain")) and self._chain_ok(sampler)
        if not chain:                               # chained: the previous sample() wrote res_a already
            ops.embed_merge(st["ids"], None, w.embed, feats, feats.shape[0] if feats is not None else 0, ws.res_a,
                            **self._embed_kw())
        if ws.route == "fin":
            layers = self._decode_layers_fx if B <= self.FUSE_MAX_B else self._decode_layers_fin
            xq, ss, tiles, n_ss = layers(st, cache, ws)
            # final RMSNorm folded into the lm_head GEMV: x' = resid*(1+w) from the last down_proj, rstd on the outputs
            logits = self._buf("d_logits", (B, w.vocab_local_pad), torch.float32)
            fa = ops.fused_args(pro_mode=ops.PRO_X_RSTD, ss_in=ss, ss_ld=tiles, ss_n=n_ss, eps=1e-6)
            lm_w, wf, nk = self._dec_w({"lm_w": w.lm_w, "lm_w13": w.lm_w13}, "lm", B)
            ops.gemm_fused(xq, lm_w, logits, fa, epi=ops.EPI_F32 | wf, M=B, bias=w.lm_bias, **nk)
            logits = logits[:, :w.vocab]
        else:
            layers = self._decode_layers_fused if ws.route == "fused" else self._decode_layers_unfused
            ns = layers(st, cache, ws)
            xn = ws.xn
            if ws.route == "unfused" and self._mx_decode(B)[1]:   # MX rows for the fp8 lm_head (it applies rstd)
                H = w.hidden
                xn = ("mx",) + ops.norm_residual_mx(ws.res_a, w.final_w, self._buf("d_x8n", (B, H), torch.uint8),
                                                    self._buf("d_xsn", (B * H // 32,), torch.uint8),
                                                    self._buf("d_ssn", (B, H // 1024), torch.float32),
                                                    partials=ws.part, nsplit=ns, write_resid=False)
            else:
                ops.norm_residual(ws.res_a, w.final_w, mode=ops.NORM_RMS, partials=ws.part, nsplit=ns, out=xn,
                                  write_resid=False)
            if self.tp > 1 and sampler is not None and not sampler.get("do_sample"):
                return self._tp_greedy(xn, st)
            logits = self.lm_head(xn, B, name="d_logits")
        if sampler is not None:
            self.sample(logits, st, sampler, advance=True, feats=feats)
        return logits

    def _tp_greedy(self, xn, st: dict) -> torch.Tensor:
        """Vocabulary-parallel greedy sampling from the normalised rows: local (max, index) pairs -> all-gather ->
        merge (advances the state).  Returns this rank's logits slice [B][vocab_local]."""
        w = self.w
        B = st["ids"].numel()
        loc = self._buf("d_logits_loc", (B, w.vocab_local_pad), torch.float32)
        self._lm_gemm(xn, B, loc)
        loc = loc[:, :w.vocab_local]
        Bp = B + (B & 1)                    # whole 16-byte exchange units (pairs of rows)
        mine = self._buf("d_pairs_loc", (Bp, 2), torch.float32)
        ops.argmax_pairs(loc, st["ws"], mine, vocab_offset=w.vocab_offset)
        pairs = self._buf("d_pairs", (self.tp, Bp, 2), torch.float32)
        self.comm.all_gather(pairs, mine)
        if Bp != B:
            pairs = self._buf("d_pairs_b", (self.tp, B, 2), torch.float32).copy_(pairs[:, :B])
        ops.argmax_merge(pairs, st["ids"], world=self.tp, hist=st["hist"], step=st["step"], pos=st["pos"],
                         kv_len=st["kv_len"])
        return loc

    # ---- what the three layer forms share: layer i's RoPE / KV-append arguments, its split-KV attention, the merge
    def _rope_kw(self, i: int, st: dict, cache: KVStore, ws) -> dict:
        """PgFusedArgs fields of layer i's decode q|k|v epilogue: RoPE at the rows' positions, K / V appended at the
        device-resident kv length (canonical and decode-order copies)."""
        w = self.w
        return dict(head_dim=w.head_dim, cos_t=ws.cos_t, sin_t=ws.sin_t, pos=st["pos"], rows_per_batch=1,
                    kc=cache.k[i], vtc=cache.vt[i], smax=cache.Smax, q_heads=w.heads, kv_heads=w.kv_heads,
                    kd=cache.kd[i], vd=cache.vd[i], **self._slot_kw(st, ws))

    @staticmethod
    def _slot_kw(st: dict, ws) -> dict:
        """Where a decode launch finds a row's kv length before its token (= its append slot): the batch's one
        kv_len word, or with per-row lengths pos[b] - 1 (slot = position - 1 for real tokens; launched with ws.sr)."""
        if ws.ragged:
            return dict(slot_dev=st["pos"], slot_base=-1)
        return dict(slot_dev=st["kv_len"], slot_base=0)

    def _attn_split(self, i: int, st: dict, cache: KVStore, ws):
        """Layer i's split-KV decode attention: the (O, m, l) partials of ws.nsplit splits of ws.SK keys."""
        w = self.w
        nh, nkv, hd = w.heads, w.kv_heads, w.head_dim
        kvd = nkv * hd
        a_args = (ws.qb, nh * hd, None, nh * hd, cache.k[i], cache.Smax * kvd, hd, kvd,
                  cache.vt[i], kvd * cache.Smax, hd * cache.Smax, cache.Smax)
        kw = dict(B=ws.B, Lq=1, Hq=nh, Hkv=nkv, D=hd, scale=1.0 / math.sqrt(hd), split_keys=ws.SK, nsplit=ws.nsplit,
                  part_o=ws.part_o, part_ml=ws.part_ml, kcap=cache.Smax, kd=cache.kd[i], vd=cache.vd[i])
        if ws.ragged:                               # row b holds pos[b] keys once its token is appended
            ops.attention_rows(*a_args, Lkv=0, lkv_rows=st["pos"], **kw)
        else:
            ops.attention(*a_args, Lkv=1, lkv_dev=st["kv_len"], **kw)

    def _combine_kw(self, st: dict, ws) -> dict:
        """PgFusedArgs fields of an o_proj GEMV that merges the split-KV partials in its prologue."""
        w = self.w
        return dict(pro_mode=ops.PRO_ATTN_COMBINE, part_o=ws.part_o, part_ml=ws.part_ml, asplit=ws.nsplit,
                    head_dim=w.head_dim, dtw=ws.dt, q_per_kv=w.heads // w.kv_heads, kv_heads=w.kv_heads,
                    akeys=ws.SK, **self._slot_kw(st, ws))

    def _decode_attn_merged(self, i: int, st: dict, cache: KVStore, ws, want_fp8: bool = False):
        """Split-KV decode attention of layer i for B > FUSE_MAX_B rows, merged: one pg_attn_decode launch, or where
        that kernel does not apply (head_dim, a cache under 64 keys, fewer than FUSED_MIN_ROUNDS rounds per split) the
        split kernel + pg_attn_combine.  Returns the o_proj's input: the rows as bf16 [B][nh*hd], or with want_fp8,
        when the one-launch kernel can write them, as (e4m3, row scales) -- no quantiser launch."""
        w = self.w
        B = ws.B
        nh, nkv, hd = w.heads, w.kv_heads, w.head_dim
        attn = self._buf("d_attn", (B, nh * hd), torch.bfloat16)
        # the one-launch kernel where the cache needs several rounds of waves (pt-896 x32: 34.3 vs 43.3 us per layer,
        # attention + merge); with one round its last split's serial merge of every partial costs more than the
        # combine launch (pt-224 x16 1.374 vs 1.350 ms/step, round 4).  Since round 5's cheaper merge tail (8 partials
        # per round trip, the four waves storing the split's partial) two rounds win too: pt-448 x16 1.348-1.351 vs
        # 1.391-1.392 ms/step (profiles/r05_fused_attn_pt448_ab.jsonl; round 4 measured 1.429 vs 1.412)
        plan = ops.decode_plan(B, nkv, cache.Smax)
        if hd in (32, 256) and cache.Smax >= 64 and plan[2] >= self.FUSED_MIN_ROUNDS:
            x8 = None
            if want_fp8 and ops.attn_decode_q8_ok(nh, nkv, hd, plan[1]):
                x8 = self._x8(B, nh * hd)
            ops.attn_decode(ws.qb, nh * hd, attn, nh * hd, cache.kd[i], cache.vd[i],
                            B=B, Lkv=0 if ws.ragged else 1, lkv_dev=st["pos"] if ws.ragged else st["kv_len"],
                            rows=ws.ragged, Hq=nh, Hkv=nkv, D=hd, scale=1.0 / math.sqrt(hd),
                            kcap=cache.Smax, part_o=ws.part_o, part_ml=ws.part_ml,
                            counters=self._zeros("d_dec_cnt", (B * nkv,), torch.int32), plan=plan,
                            q8=x8[0] if x8 else None, q8_scale=x8[1] if x8 else None)
            return x8 or attn
        self._attn_split(i, st, cache, ws)
        ops.attn_combine(ws.part_o, ws.part_ml, attn, nh * hd, B=B, Hq=nh, Hkv=nkv, D=hd, nsplit=ws.nsplit)
        return attn

    def fx_status(self) -> torch.Tensor:
        """The fixed-point residual's status word (PgFusedArgs.status): an FX_ADD launch sets it when a value is
        non-finite or beyond the accumulator's +-2^31 range (saturated, so the step's results are invalid)."""
        return self._zeros("d_fx_status", (1,), torch.int32)

    def check_numerics(self):
        """Raise if a decode step's fixed-point residual overflowed or received a NaN / Inf (one host read)."""
        t = self._ws.get("d_fx_status")
        if t is not None and int(t.item()):
            t.zero_()
            raise FloatingPointError("decode residual: a non-finite or out-of-range (|v| >= 2^31) value reached the "
                                     "fixed-point accumulator; the generated tokens are invalid")

    def _zeros(self, name, shape, dtype):
        """Persistent zero-initialised buffer (e.g. self-resetting arrival tickets)."""
        t = self._ws.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.zeros(*shape, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t

    def _decode_layers_fused(self, st: dict, cache: KVStore, ws) -> int:
        """Decode layers for B <= FUSE_MAX_B under tensor parallelism (or USE_FIN off), 5 launches each:
        [RMSNorm + q|k|v GEMV + RoPE + KV append] -> split-KV attention -> [attention merge + o GEMV (split-K
        partials)] -> [RMSNorm + gate/up GEMV + gelu*mul] -> down GEMV (split-K partials).  The residual stream
        ping-pongs between two fp32 buffers; the RMSNorm prologues add the previous GEMV's split-K partials
        (deterministic order).  Returns the slab count the final norm must add."""
        w = self.w
        B, res_a, res_b, part = ws.B, ws.res_a, ws.res_b, ws.part
        ns = 0
        for i, Lw in enumerate(w.tl):
            fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, resid_in=res_a, resid_out=res_b, partials=part, nsplit=ns,
                                norm_w=Lw["in_w"], eps=1e-6, **self._rope_kw(i, st, cache, ws))
            ops.gemm_fused(None, Lw["qkv_w"], ws.qb, fa, epi=ops.EPI_QKV_ROPE | w.wflag | ws.sr, M=B)
            self._attn_split(i, st, cache, ws)
            fa = ops.fused_args(**self._combine_kw(st, ws))
            ops.gemm_fused(None, Lw["o_w"], part, fa, epi=ops.EPI_F32 | w.wflag | ws.sr, M=B, ksplit=ws.so)
            n_o = self._allreduce_slabs(part, ws.so)
            fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, resid_in=res_b, resid_out=res_a, partials=part, nsplit=n_o,
                                norm_w=Lw["post_w"], eps=1e-6)
            ops.gemm_fused(None, Lw["gu_w"], ws.h, fa, epi=ops.EPI_BF16_GELU_MUL | w.wflag, M=B)
            ops.gemm(ws.h, Lw["down_w"], part, epi=ops.EPI_F32 | w.wflag, ksplit=ws.sd)
            ns = self._allreduce_slabs(part, ws.sd)
        return ns

    def _dec_w(self, d, name: str, B: int, ksplit: int = 1):
        """(W, layout flag, N / K keywords) of the decode launch of d[name + "_w"] at B rows on the fx / fin routes: the
        13-bit pack (its 12-bit form for a launch in w12_forms) when the switch is on, the matrix has one, the launch is
        a B <= FUSE_MAX_B form and every wave of a split owns whole 128-k blocks; else the bf16 fragment pack."""
        W = d[name + "_w"]
        p13 = d.get(name + "_w13")
        if (self.W13 and p13 is not None and name in self.W13_FORMS and B <= self.FUSE_MAX_B and self.tp == 1
                and (W.shape[1] // 64) % (8 * ksplit) == 0):
            f12 = ops.W_FRAG12 if name in getattr(self.w, "w12_forms", ()) else 0
            return p13, ops.W_FRAG13 | f12, dict(N=W.shape[0], K=W.shape[1])
        return W, self.w.wflag, {}

    def _decode_layers_fx(self, st: dict, cache: KVStore, ws):
        """Decode layers (single rank, bf16, B <= FUSE_MAX_B), 5 launches each, on a fixed-point residual: o_proj and
        down_proj add their split-K partials into an int64 accumulator with integer atomics (EPI_FX_ADD: the sum is
        exact, so decode is bit-reproducible run to run), and every GEMV that follows normalises the accumulator in its
        prologue (PRO_RMSNORM, fx=).  Layer 0's q|k|v GEMV reads the embedding rows instead and clears the accumulator;
        layer 0's o_proj folds those rows in, so from there on the accumulator holds the whole residual.  o_proj also
        merges the split-KV partials in its prologue.  The last layer's down_proj finalises in-kernel (EPI_F32_FIN with
        fx=: adds the accumulator, clears it, writes x' = bf16(resid*(1+w_final)) and per-tile sums of squares) for
        the lm_head.  gate/up, down and the lm_head stream the 13- / 12-bit weight packs (_dec_w).
        Returns (x', sums of squares, their row stride, entries per row) of the final norm for the lm_head."""
        w = self.w
        B, res = ws.B, ws.res_a
        tiles = (w.hidden + 15) // 16
        fx = self._zeros("d_fx", (B, w.hidden), torch.int64)    # zero between steps: the finalising down clears it
        status = self.fx_status()                               # set by an FX_ADD launch given an unholdable value
        xq = self._buf("d_xq", (B, w.hidden), torch.bfloat16)
        ss = self._buf("d_ss_d", (B, tiles), torch.float32)
        for i, Lw in enumerate(w.tl):
            fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, nsplit=0, norm_w=Lw["in_w"], eps=1e-6,
                                **self._rope_kw(i, st, cache, ws))
            if i == 0:
                # the step starts from a zero accumulator whatever an earlier (interrupted) step left in it: layer 0's
                # q|k|v GEMV does not read it and clears it before layer 0's o_proj adds into it
                fa.resid_in, fa.amax_zero, fa.amax_zero_n = res.data_ptr(), fx.data_ptr(), fx.numel() * 2
            else:
                fa.fx = fx.data_ptr()
            qkv_w, wf, nk = self._dec_w(Lw, "qkv", B)
            ops.gemm_fused(None, qkv_w, ws.qb, fa, epi=ops.EPI_QKV_ROPE | wf | ws.sr, M=B, **nk)
            self._attn_split(i, st, cache, ws)
            fa = ops.fused_args(resid_in=res if i == 0 else None, status=status, **self._combine_kw(st, ws))
            o_w, wf, nk = self._dec_w(Lw, "o", B, ws.so)
            ops.gemm_fused(None, o_w, fx, fa, epi=ops.EPI_FX_ADD | wf | ws.sr, M=B, ksplit=ws.so, **nk)
            fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, fx=fx, nsplit=0, norm_w=Lw["post_w"], eps=1e-6)
            gu_w, wf, nk = self._dec_w(Lw, "gu", B)
            ops.gemm_fused(None, gu_w, ws.h, fa, epi=ops.EPI_BF16_GELU_MUL | wf, M=B, **nk)
            down_w, wf, nk = self._dec_w(Lw, "down", B, ws.sd)
            if i + 1 < len(w.tl):
                ops.gemm_fused(ws.h, down_w, fx, ops.fused_args(status=status), epi=ops.EPI_FX_ADD | wf, M=B,
                               ksplit=ws.sd, **nk)
            else:
                fa = ops.fused_args(fin_cnt=self._zeros("d_fin_cnt", (tiles,), torch.int32), fin_resid=res, ss_out=ss,
                                    ss_ld=tiles, fin_x=xq, norm_w=w.final_w, fx=fx)
                ops.gemm_fused(ws.h, down_w, ws.part, fa, epi=ops.EPI_F32_FIN | wf, M=B, ksplit=ws.sd, **nk)
        return xq, ss, tiles, tiles if B <= 4 else (tiles + 1) // 2

    def _decode_layers_fin(self, st: dict, cache: KVStore, ws):
        """Decode layers (single rank, bf16, more than FUSE_MAX_B and up to 16 rows), 5 launches each, with in-kernel
        split-K finalisation: o_proj and down_proj add their split-K slabs into the residual in place (the
        last-arriving split of each 16-column tile, EPI_F32_FIN), and write x' = bf16(resid*(1+w_next)) plus per-tile
        sums of squares; the next GEMV (gate/up, the next layer's q|k|v, finally the lm_head) reads x' like a plain
        activation and scales its outputs by rstd (PRO_X_RSTD; RMSNorm: W.(x*rstd*(1+w)) = rstd * W.(x*(1+w))).  Only
        layer 0's q|k|v GEMV normalises itself (PRO_RMSNORM, the embedding rows).  The split-KV merge runs as its own
        kernel (_decode_attn_merged: folded into every o_proj workgroup it would be recomputed per workgroup), and
        above 4 rows the GEMVs run two 16-column tiles per workgroup, so the sums of squares come one per tile pair.
        Returns (x', sums of squares, their row stride, entries per row) of the final norm for the lm_head."""
        w = self.w
        B, res, part, wflag = ws.B, ws.res_a, ws.part, w.wflag
        tiles = (w.hidden + 15) // 16
        n_ss = tiles if B <= 4 else (tiles + 1) // 2            # one entry per GEMV workgroup
        cnt = self._zeros("d_fin_cnt", (tiles,), torch.int32)
        ss_o = self._buf("d_ss_o", (B, tiles), torch.float32)
        ss_d = self._buf("d_ss_d", (B, tiles), torch.float32)
        xq = self._buf("d_xq", (B, w.hidden), torch.bfloat16)
        for i, Lw in enumerate(w.tl):
            rope = self._rope_kw(i, st, cache, ws)
            if i == 0:
                fa = ops.fused_args(pro_mode=ops.PRO_RMSNORM, resid_in=res, nsplit=0, norm_w=Lw["in_w"], eps=1e-6, **rope)
                ops.gemm_fused(None, Lw["qkv_w"], ws.qb, fa, epi=ops.EPI_QKV_ROPE | wflag | ws.sr, M=B)
            else:
                fa = ops.fused_args(pro_mode=ops.PRO_X_RSTD, ss_in=ss_d, ss_ld=tiles, ss_n=n_ss, eps=1e-6, **rope)
                ops.gemm_fused(xq, Lw["qkv_w"], ws.qb, fa, epi=ops.EPI_QKV_ROPE | wflag | ws.sr, M=B)
            attn = self._decode_attn_merged(i, st, cache, ws)
            fa = ops.fused_args(fin_cnt=cnt, fin_resid=res, ss_out=ss_o, ss_ld=tiles, fin_x=xq, norm_w=Lw["post_w"])
            ops.gemm_fused(attn, Lw["o_w"], part, fa, epi=ops.EPI_F32_FIN | wflag, M=B, ksplit=ws.so)
            fa = ops.fused_args(pro_mode=ops.PRO_X_RSTD, ss_in=ss_o, ss_ld=tiles, ss_n=n_ss, eps=1e-6)
            ops.gemm_fused(xq, Lw["gu_w"], ws.h, fa, epi=ops.EPI_BF16_GELU_MUL | wflag, M=B)
            nxt_w = w.tl[i + 1]["in_w"] if i + 1 < len(w.tl) else w.final_w
            fa = ops.fused_args(fin_cnt=cnt, fin_resid=res, ss_out=ss_d, ss_ld=tiles, fin_x=xq, norm_w=nxt_w)
            ops.gemm_fused(ws.h, Lw["down_w"], part, fa, epi=ops.EPI_F32_FIN | wflag, M=B, ksplit=ws.sd)
        return xq, ss_d, tiles, n_ss

    def _split_keys(self, B: int, Smax: int) -> int:
        """Keys per decode-attention split: 32 (one MFMA block) at small batch; at B > FUSE_MAX_B (separate
        merge kernel) whole multiples of 32 such that B * splits stays near DECODE_SPLIT_TARGET -- fewer (O, m, l)
        partials to write and merge once the batch alone fills the chip."""
        SK = self.DECODE_SPLIT_KEYS
        if B <= self.FUSE_MAX_B:
            return self.DECODE_SPLIT_KEYS_SMALL
        blocks = (Smax + SK - 1) // SK
        mult = max(1, min(8, (B * blocks) // self.DECODE_SPLIT_TARGET))
        # a power of two: 2 / 4 / 8-block splits run one wave per block, merged in LDS (attn_decode_wg_kernel)
        return SK * (1 << (mult.bit_length() - 1))

    def _decode_layers_unfused(self, st: dict, cache: KVStore, ws) -> int:
        """Decode layers for B > FUSE_MAX_B: the RMSNorm and the split-KV merge run once as their own
        kernels (fused into every GEMV workgroup they would be recomputed B-fold per workgroup).  17..32 fp8 rows run
        on the fp8 GEMVs, with MX h / MX norms where _mx_decode allows.  Returns the slab count the final norm must
        add."""
        w = self.w
        B, res, part, h = ws.B, ws.res_a, ws.part, ws.h
        I, H = w.inter, w.hidden
        mx, mxn = self._mx_decode(B)
        if mx:
            h8 = self._buf("d_h8", (B, I), torch.uint8)
            hs = self._buf("d_hs", (B * I // 32,), torch.uint8)
        if mxn:
            x8n = self._buf("d_x8n", (B, H), torch.uint8)
            xsn = self._buf("d_xsn", (B * H // 32,), torch.uint8)
            ssn = self._buf("d_ssn", (B, H // 1024), torch.float32)
        ns = 0
        for i, Lw in enumerate(w.tl):
            fa = ops.fused_args(**self._rope_kw(i, st, cache, ws))
            if mxn:                                 # MX rows of x*(1+w); the q|k|v GEMV applies rstd
                ops.norm_residual_mx(res, Lw["in_w"], x8n, xsn, ssn, partials=part, nsplit=ns)
                ops.gemm8(x8n, None, Lw["qkv_w8f"], Lw["qkv_s8"], ws.qb, epi=ops.EPI_QKV_ROPE | ws.sr, M=B, fa=fa,
                          frag=True, mx_in=xsn, ss_in=ssn)
            else:
                xin = self._norm(res, Lw["in_w"], part, ns, ws.xn, B)
                self._lin(xin, Lw, "qkv", ws.qb, ops.EPI_QKV_ROPE | ws.sr, B, fa=fa)
            attn = self._decode_attn_merged(i, st, cache, ws, want_fp8=self._fp8_rows(B))
            self._lin(attn, Lw, "o", part, ops.EPI_F32, B, ksplit=ws.so)
            n_o = self._allreduce_slabs(part, ws.so)
            if mxn:                                 # MX norm -> gate/up (rstd, MX h)
                ops.norm_residual_mx(res, Lw["post_w"], x8n, xsn, ssn, partials=part, nsplit=n_o)
                ops.gemm8(x8n, None, Lw["gu_w8f"], Lw["gu_s8"], h8, epi=ops.EPI_BF16_GELU_MUL, M=B, frag=True,
                          mx_in=xsn, ss_in=ssn, mx_out=hs)
            else:
                xin = self._norm(res, Lw["post_w"], part, n_o, ws.xn, B)
                if mx:                              # fp8 rows -> gate/up writing MX h: e4m3 + block scales
                    x8, xs = xin
                    ops.gemm8(x8, xs, Lw["gu_w8f"], Lw["gu_s8"], h8, epi=ops.EPI_BF16_GELU_MUL, M=B, frag=True,
                              mx_out=hs)
                else:
                    self._lin(xin, Lw, "gu", h, ops.EPI_BF16_GELU_MUL, B)
            if mx:                                  # MX h straight from gate/up into down
                ops.gemm8(h8, None, Lw["down_w8f"], Lw["down_s8"], part, epi=ops.EPI_F32, M=B, ksplit=ws.sd,
                          frag=True, mx_in=hs)
            else:
                self._lin(h, Lw, "down", part, ops.EPI_F32, B, ksplit=ws.sd)
            ns = self._allreduce_slabs(part, ws.sd)
        return ns

    def sample(self, logits: torch.Tensor, st: dict, sampler: dict, advance: bool,
               feats: Optional[torch.Tensor] = None):
        """Next ids from logits [B][V] (greedy or top-p); advance=True also moves pos / kv_len on.  A chained
        state (decode_state) also gets the next step's input rows: pass the request's image features.
        sampler["grammar"] (grammar_state): pg_dfa_mask on the logits, in place, before the sampler that would have run
        anyway, and pg_dfa_advance on the ids it wrote -- two small launches, nothing leaves the device."""
        if sampler.get("beam") is not None:
            return self._beam_sample(logits, st, sampler["beam"], advance)
        gr = sampler.get("grammar")
        if gr is not None:      # constrained rows: -inf over what their DFA state does not allow, then the same sampler
            ops.dfa_mask(logits, gr["cls"], gr["trans"], gr["state"])
        kw = dict(hist=st["hist"], step=st["step"])
        if advance:     # (per-row lengths: pos[b] is the row's length too, and the samplers leave a null kv_len alone)
            kw.update(pos=st["pos"], kv_len=None if st.get("ragged") else st["kv_len"])
        if st.get("chain") and self._chain_ok(sampler):
            w = self.w
            B = st["ids"].numel()
            ops.argmax_embed(logits, st["ids"], st["ws"], w.embed, feats, feats.shape[0] if feats is not None else 0,
                             self._buf("d_res_a", (B, w.hidden), torch.float32), **self._embed_kw(), **kw)
        elif sampler.get("do_sample"):
            ops.topp_sample(logits, st["ids"], sampler["uniforms"], temperature=sampler["temperature"],
                            top_p=sampler["top_p"], **kw)
        else:
            ops.argmax(logits, st["ids"], st["ws"], **kw)
        if gr is not None:      # ... and the states follow the tokens picked
            ops.dfa_advance(gr["state"], st["ids"], gr["cls"], gr["trans"], gr["err"])

    def _beam_sample(self, logits: torch.Tensor, st: dict, bm: dict, advance: bool):
        """The beam sampler: pg_beam_select on the step's logits (ids, parents, scores, finished flags, both histories
        and the state advance), then -- once the step has appended a key -- pg_kv_beam_gather, so that row r's
        generated keys and values are those of the hypothesis it now continues."""
        ragged = bool(st.get("ragged"))
        kw = dict(hist_tok=st["hist"], hist_parent=bm["hist_parent"], step=st["step"], flag=bm["flag"])
        if advance:
            kw.update(pos=st["pos"], kv_len=None if ragged else st["kv_len"])
        ops.beam_select(logits, bm["cum"], bm["finished"], st["ids"], bm["parent"], bm["ws"], W=bm["W"],
                        V=self.w.vocab, stop_token=bm["stop_token"], pad_token=bm["pad_token"], **kw)
        bm["logits"] = logits                       # (a static buffer: the trace copies it after each step)
        if advance:
            c = bm["cache"]
            ops.kv_beam_gather(c.k, c.vt, c.kd, c.vd, bm["parent"], bm["base"],
                               st["pos"] if ragged else st["kv_len"], bm["scratch"], kv_heads=c.kv_heads,
                               len_rows=ragged, len_base=-1 if ragged else 0, S_scr=bm["S_scr"])

    # ------------------------------------------------------------------ full request
    def prefill_request(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, attention_mask: torch.Tensor,
                        max_new_tokens: int, feats: Optional[torch.Tensor] = None):
        """Vision + merge + Gemma prefill; returns (cache, feats, last-position logits [B][V], next positions).
        The mask must be right-padded (mask_lengths); row b is then a request of its first len_b tokens: its keys stop
        at len_b (per-row prefill attention), its logits come from position len_b - 1, and the returned cache is marked
        ragged when any len_b < L, so decode_state / decode_step append and attend per row.  An all-ones mask takes the
        same launches as before."""
        B, L = input_ids.shape
        lens_h = mask_lengths(attention_mask)                   # host check, before any launch
        ragged = bool((lens_h < L).any())
        if ragged and self.tp > 1:
            raise NotImplementedError("prompts of different lengths in one batch (a padded attention_mask) are not "
                                      "supported under tensor parallelism (tp > 1); pad-free batches are")
        if feats is None:
            feats = self.vision(pixel_values)
        cache = self.new_cache(B, L + max_new_tokens + 1)
        resid = self._buf("p_resid", (B * L, self.w.hidden), torch.float32)
        self.embed_merge(input_ids.to(self.device), feats, resid)
        am = attention_mask.to(self.device)
        pos = am.cumsum(-1).masked_fill(am == 0, 1)                       # modeling_paligemma.py:195
        lens = lens_h.to(device=self.device, dtype=torch.int32).contiguous() if ragged else None
        rows = torch.arange(B, device=self.device, dtype=torch.int32) * L + (lens - 1 if ragged else L - 1)
        logits, _ = self.gemma_prefill(resid, pos, cache, B, L, logits_rows=rows.contiguous(), kv_rows=lens)
        nxt = am.sum(-1).to(torch.int32) + 1                              # modeling_paligemma.py:189
        return cache, feats, logits, nxt

    # ------------------------------------------------------------------ scoring a given answer
    SCORE_CHUNK_ROWS = 128  # answer rows per lm_head + token_logprob launch pair: one reused [chunk][V] fp32 buffer
    # rows every score lm_head launch computes at least: one more than the GEMV takes, so always the tile GEMM (score())
    _SCORE_MIN_M = ops.GEMV_MAX_M + 1

    @staticmethod
    def score_spans(attention_mask: torch.Tensor, token_type_ids: torch.Tensor):
        """(prefix lengths, row lengths), int64 [B] on the host, of a scoring batch: row b is [prefix_b | suffix_b | pad]
        with the mask right-padded (mask_lengths) and token_type_ids 0 over the prefix, 1 over the suffix, 0 over the
        padding.  Raises ValueError -- before anything is launched -- for type ids whose ones are not one run ending at
        the row's length, for a row without a suffix, and for a suffix that starts at position 0."""
        lens = mask_lengths(attention_mask)
        if tuple(token_type_ids.shape) != tuple(attention_mask.shape):
            raise ValueError(f"token_type_ids {tuple(token_type_ids.shape)} must match attention_mask "
                             f"{tuple(attention_mask.shape)}")
        t = token_type_ids.detach().to("cpu") != 0
        n1 = t.sum(-1)
        if bool((n1 == 0).any()):
            raise ValueError(f"token_type_ids: row {int((n1 == 0).nonzero()[0])} has an empty suffix (no token of type 1)")
        prefix = lens - n1
        idx = torch.arange(t.shape[1])[None, :]
        want = (idx >= prefix[:, None]) & (idx < lens[:, None])
        if not torch.equal(t, want):
            bad = int((t != want).any(-1).nonzero()[0])
            raise ValueError(f"token_type_ids: row {bad}'s ones are not one contiguous run ending at the row's length "
                             f"{int(lens[bad])} (prefix 0s, suffix 1s, padding 0s)")
        if bool((prefix < 1).any()):
            raise ValueError(f"token_type_ids: row {int((prefix < 1).nonzero()[0])}'s suffix starts at position 0 "
                             "(nothing to condition the first answer token on)")
        return prefix, lens

    def score(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, attention_mask: torch.Tensor,
              token_type_ids: torch.Tensor, return_logits: bool = False) -> dict:
        """Log-probabilities of given answers: row b of input_ids is [prefix_b | suffix_b | pad] (image + prompt, then
        the answer; score_spans' layout).  One prefix-LM prefill over all rows -- prefix positions attend one another,
        answer positions causally (ops.attention_prefix), positions as in prefill_request -- then the final norm, the
        lm_head and pg_token_logprob on the rows that predict an answer token only: position p predicts token p + 1,
        so row b contributes positions prefix_b - 1 .. len_b - 2.  Those rows run in chunks of SCORE_CHUNK_ROWS through
        one logits buffer (a long answer never holds rows x V fp32), every launch on the bf16 tile GEMM with at least
        ops.GEMV_MAX_M + 1 = 17 rows (a chunk shorter than that also runs the rows after it -- the row list is padded
        by 16 -- instead of switching to the GEMV, whose sums differ in the last bits): the result does not depend on
        the chunk size.  The price is a short answer's: 17 lm_head rows where one would do (scripts/tune/score_bench.py
        times both).

        Returns {"logprobs": fp32 [B][S_max], 0 past a row's answer; "top1": int64 [B][S_max] the model's own greedy
        token at each answer position, the pad id past it; "suffix_lens": int64 [B]; with return_logits also "logits":
        fp32 [sum S_b][V], row b's answer rows after row b - 1's}."""
        B, L = input_ids.shape
        prefix_h, lens_h = self.score_spans(attention_mask, token_type_ids)       # host checks, before any launch
        if self.tp > 1:
            raise NotImplementedError("score() is not supported under tensor parallelism (tp > 1)")
        w = self.w
        dev = self.device
        suf = lens_h - prefix_h
        S_max, R = int(suf.max()), int(suf.sum())
        b_of = torch.repeat_interleave(torch.arange(B), suf)                       # [R] batch row of each answer token
        j_of = torch.arange(R) - torch.repeat_interleave(torch.cumsum(suf, 0) - suf, suf)     # its index in the answer
        p_of = prefix_h[b_of] + j_of                                               # its position in the row
        ids = input_ids.to(dev)
        targets = ids[b_of.to(dev), p_of.to(dev)].to(torch.int64).contiguous()
        pad_rows = max(0, self._SCORE_MIN_M - 1)        # so that a last chunk of one row still has 17 rows to run
        row_map = torch.cat([b_of * L + p_of - 1, torch.zeros(pad_rows, dtype=torch.int64)])
        row_map = row_map.to(device=dev, dtype=torch.int32).contiguous()

        feats = self.vision(pixel_values)
        cache = self.new_cache(B, L + 1)
        resid = self._buf("p_resid", (B * L, w.hidden), torch.float32)
        self.embed_merge(ids, feats, resid)
        am = attention_mask.to(dev)
        pos = am.cumsum(-1).masked_fill(am == 0, 1)                                # modeling_paligemma.py:195
        _, _, xf = self.gemma_prefill(resid, pos, cache, B, L, logits_rows=row_map, want_logits=False,
                                      kv_rows=lens_h.to(device=dev, dtype=torch.int32).contiguous(),
                                      prefix_rows=prefix_h.to(device=dev, dtype=torch.int32).contiguous(),
                                      return_rows=True)                          # xf: the normalised rows [R + pad][H]

        logprob = torch.empty(R, dtype=torch.float32, device=dev)
        top1 = torch.empty(R, dtype=torch.int64, device=dev)
        out_logits = torch.empty(R, w.vocab, dtype=torch.float32, device=dev) if return_logits else None
        chunk = max(1, int(self.SCORE_CHUNK_ROWS))
        buf = self._buf("score_logits", (max(chunk, self._SCORE_MIN_M), w.vocab_local_pad), torch.float32)
        ws = self._buf("score_ws", (ops.token_logprob_workspace(chunk),), torch.uint8)
        for r0 in range(0, R, chunk):
            n = min(chunk, R - r0)
            m = max(n, self._SCORE_MIN_M)
            ops.gemm(xf[r0:r0 + m], w.lm_w, buf[:m], epi=ops.EPI_F32 | w.wflag, bias=w.lm_bias)
            ops.token_logprob(buf[:n], targets[r0:r0 + n], logprob[r0:r0 + n], top1[r0:r0 + n], ws, V=w.vocab)
            if return_logits:
                out_logits[r0:r0 + n].copy_(buf[:n, :w.vocab])
        pad = self.pad_id if self.pad_id >= 0 else 0
        lp = torch.zeros(B, S_max, dtype=torch.float32, device=dev)
        t1 = torch.full((B, S_max), pad, dtype=torch.int64, device=dev)
        lp[b_of.to(dev), j_of.to(dev)] = logprob
        t1[b_of.to(dev), j_of.to(dev)] = top1
        out = {"logprobs": lp, "top1": t1, "suffix_lens": suf.clone()}
        if return_logits:
            out["logits"] = out_logits
        return out

    def generate(self, input_ids, pixel_values, attention_mask, max_new_tokens: int, do_sample=False,
                 temperature=0.8, top_p=0.9, uniforms=None, stop_token: Optional[int] = 1, use_graph=True,
                 check_every: Optional[int] = None, pad_token: int = 0, return_list: bool = False,
                 grammar=None, grammar_start=None):
        """test_inference's loop (inference.py:45-82) for B >= 1 rows.

        B = 1: ids [1][n], stopping after EOS like the reference.  B > 1 (the reference asserts B = 1,
        SURVEY §8(f2)): every row decodes in the same static-shape graph until ALL rows have produced
        `stop_token` (checked every `check_every` steps, default 8, one host sync each) or max_new_tokens;
        a row's tokens after its EOS are replaced by `pad_token` in the [B][n] result, or dropped when
        return_list=True (a list of per-row id lists, each ending at its EOS).  Rows of different prompt lengths:
        a right-padded attention_mask (prefill_request); each row then generates what it generates alone at B = 1.

        grammar (a pghip.grammar.TokenDFA): constrained decoding.  Every token, the first included, is picked among
        those the row's DFA state allows -- the others' logits are set to -inf on the device before the greedy or
        top-p sampler runs (pg_dfa_mask), and the state follows the pick (pg_dfa_advance); the step stays one graph.
        grammar_start: the start state, an int or one per row; -1 leaves a row unconstrained (it generates what it
        generates without a grammar); default: the grammar's single start state.  A grammar whose cls does not cover
        the vocabulary, a start state outside {-1} U [0, S) and a start list of the wrong length raise ValueError
        before anything is launched; tp > 1 raises NotImplementedError.  Should a constrained row's allowed logits all
        be NaN, the sampler's fallback token breaks the grammar: RuntimeError after the loop."""
        B = input_ids.shape[0]
        if check_every is None:
            check_every = 1 if B == 1 else 8
        starts = self.grammar_args(grammar, grammar_start, B, self.w.vocab)     # host checks, before any launch
        if grammar is not None and self.tp > 1:
            raise NotImplementedError("constrained decoding (grammar=) is not supported under tensor parallelism "
                                      "(tp > 1)")
        cache, feats, logits, nxt = self.prefill_request(input_ids, pixel_values, attention_mask, max_new_tokens)
        sampler = dict(do_sample=do_sample, temperature=temperature, top_p=top_p)
        st = self.decode_state(B, cache, nxt, max_new_tokens, sampler=sampler)
        if grammar is not None:
            sampler["grammar"] = self.grammar_state(grammar, starts)
        if do_sample:
            if uniforms is None:
                uniforms = torch.rand(max_new_tokens + 1, B)
            sampler["uniforms"] = uniforms.to(device=self.device, dtype=torch.float32).contiguous()
        self.sample(logits, st, sampler, advance=False, feats=feats)     # token 1 from the prefill logits
        n = 1
        step_fn = None
        if use_graph and self.comm.capturable:
            try:
                step_fn = self._graph_step(st, cache, feats, sampler)
            except CaptureUnsupported:
                # a collective that cannot be captured (an all-reduce larger than the xGMI exchange buffer):
                # _graph_step restored the state before capturing and a failed capture runs nothing, so the
                # eager steps start from the same state.  Any other error propagates.
                torch.cuda.synchronize()
                step_fn = None
        if step_fn is None:
            step_fn = lambda: self.decode_step(st, cache, feats, sampler)  # noqa: E731
        while n < max_new_tokens:
            if stop_token is not None and n % check_every == 0:
                if B == 1:
                    if int(st["ids"][0]) == stop_token:                   # inference.py:73-74
                        break
                elif bool((st["hist"][:n] == stop_token).any(0).all()):   # every row has finished
                    break
            step_fn()
            n += 1
        hist = st["hist"][:n].t().contiguous().cpu()
        self.check_numerics()
        if grammar is not None and int(sampler["grammar"]["err"].item()):
            raise RuntimeError("constrained decoding: a sampled token was not allowed by its row's grammar state (the "
                               "row's allowed logits were all NaN); the generated tokens are invalid")
        if hasattr(self.comm, "check"):
            self.comm.check()              # an xGMI exchange that timed out leaves meaningless sums: raise
        if stop_token is None:
            return [r.tolist() for r in hist] if return_list else hist
        rows = []
        for r in hist.tolist():
            rows.append(r[: r.index(stop_token) + 1] if stop_token in r else r)
        if return_list:
            return rows
        if B == 1:
            return torch.tensor(rows, dtype=torch.int64)
        out = torch.full((B, max(len(r) for r in rows)), pad_token, dtype=torch.int64)
        for b, r in enumerate(rows):
            out[b, : len(r)] = torch.tensor(r, dtype=torch.int64)
        return out

    @staticmethod
    def grammar_args(grammar, grammar_start, B: int, vocab: int):
        """Host checks of generate's grammar arguments (ValueError before anything is launched); returns the B start
        states, or None without a grammar."""
        if grammar is None:
            if grammar_start is not None:
                raise ValueError("grammar_start given without a grammar")
            return None
        if len(grammar.cls) != vocab:
            raise ValueError(f"the grammar classifies {len(grammar.cls)} token ids, the model's vocabulary has {vocab}")
        if grammar_start is None:
            starts = [grammar.start] * B
        elif isinstance(grammar_start, (list, tuple)):
            starts = list(grammar_start)
            if len(starts) != B:
                raise ValueError(f"grammar_start lists {len(starts)} start states for {B} rows")
        else:
            starts = [grammar_start] * B
        for s in starts:
            if isinstance(s, bool) or not isinstance(s, int) or not -1 <= s < grammar.S:
                raise ValueError(f"grammar_start {s!r}: a start state is -1 (a free row) or in [0, {grammar.S})")
        return starts

    def grammar_state(self, grammar, starts) -> dict:
        """What sample() needs of a grammar, on the device: the two tables (uploaded once per call), one state word per
        row and the error word."""
        dev = self.device
        return dict(cls=torch.from_numpy(grammar.cls).to(dev).contiguous(),
                    trans=torch.from_numpy(grammar.trans).to(dev).contiguous(),
                    state=torch.tensor(starts, dtype=torch.int32, device=dev),
                    err=torch.zeros(1, dtype=torch.int32, device=dev))

    @staticmethod
    def beam_args(num_beams, num_return_sequences, max_new_tokens, vocab: int, length_penalty=1.0):
        """Host checks of generate_beam's arguments (ValueError before anything is launched)."""
        if not isinstance(num_beams, int) or not 1 <= num_beams <= ops.BEAM_MAX_W:
            raise ValueError(f"num_beams must be an integer in 1..{ops.BEAM_MAX_W}, got {num_beams!r}")
        if num_beams > vocab:
            raise ValueError(f"num_beams {num_beams} exceeds the vocabulary ({vocab})")
        if not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"num_return_sequences must be in 1..num_beams = {num_beams}, got {num_return_sequences!r}")
        if not isinstance(max_new_tokens, int) or max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens!r}")
        if not math.isfinite(float(length_penalty)):
            raise ValueError(f"length_penalty must be finite, got {length_penalty!r}")

    @staticmethod
    def beam_backtrack(hist_tok, hist_parent, row: int) -> list:
        """The tokens of the hypothesis that ends in `row` after the last recorded step: hist_tok / hist_parent are
        [steps][rows] lists (or arrays), parents global row indices."""
        out, cur = [], row
        for t in range(len(hist_tok) - 1, -1, -1):
            out.append(int(hist_tok[t][cur]))
            cur = int(hist_parent[t][cur])
        return out[::-1]

    def beam_begin(self, input_ids, pixel_values, attention_mask, max_new_tokens: int, W: int, stop_token=1,
                   pad_token: int = 0, lens_h=None):
        """What generate_beam sets up before its loop: the prefill of the B prompts, the B * W-row cache whose row
        bW + w is prompt b's (KVStore.repeat_rows), the decode state, the beam sampler (scores, finished flags,
        parents, the parent history, the selection workspace and the gather's scratch), and the first selection, on
        the prefill logits.  Returns (state, cache, image features, sampler): decode_step(state, cache, feats, sampler)
        is then one beam step (scripts/tune/beam_bench.py times it)."""
        w, dev = self.w, self.device
        lens_h = mask_lengths(attention_mask) if lens_h is None else lens_h
        rows = input_ids.shape[0] * W
        cache0, feats, logits0, nxt = self.prefill_request(input_ids, pixel_values, attention_mask, max_new_tokens)
        cache = cache0.repeat_rows(W)
        del cache0
        S_scr = _rup(max_new_tokens + 1, 32) + 32       # ceil32(base + new) - floor32(base) for any base
        base_h = lens_h.repeat_interleave(W)
        lo = int(base_h.min()) // 32 * 32
        bm = dict(W=W, stop_token=stop_token, pad_token=int(pad_token), cache=cache, S_scr=S_scr,
                  cum=torch.full((rows,), float("-inf"), dtype=torch.float32, device=dev),
                  finished=torch.zeros(rows, dtype=torch.int32, device=dev),
                  parent=torch.zeros(rows, dtype=torch.int32, device=dev),
                  hist_parent=torch.zeros(max_new_tokens + 1, rows, dtype=torch.int32, device=dev),
                  flag=torch.zeros(1, dtype=torch.int32, device=dev),
                  base=base_h.to(device=dev, dtype=torch.int32).contiguous(),
                  ws=torch.empty(ops.beam_select_workspace(rows, W), dtype=torch.uint8, device=dev),
                  scratch=torch.empty(ops.kv_beam_gather_scratch(w.t_layers, rows, S_scr, cache.kv_dim),
                                      dtype=torch.bfloat16, device=dev),
                  # what the first decode step's gather can touch (the graph warm-up restores it)
                  warm_window=(lo, min(cache.Smax, _rup(int(base_h.max()) + 1, 32))))
        bm["cum"][::W] = 0.0
        sampler = dict(do_sample=False, beam=bm)
        st = self.decode_state(rows, cache, nxt.repeat_interleave(W), max_new_tokens, sampler=sampler)
        # the first selection, on the prefill logits (each prompt's row given to all its beams; only beam 0 can win)
        self.sample(logits0[:, :w.vocab].repeat_interleave(W, dim=0).contiguous(), st, sampler, advance=False)
        return st, cache, feats, sampler

    def generate_beam(self, input_ids, pixel_values, attention_mask, max_new_tokens: int, num_beams: int,
                      length_penalty: float = 1.0, num_return_sequences: int = 1, stop_token: Optional[int] = 1,
                      pad_token: int = 0, use_graph=True, check_every: Optional[int] = None,
                      return_trace: bool = False) -> dict:
        """Beam search for B >= 1 right-padded prompts (as generate takes them), W = num_beams hypotheses each.

        The frozen-beam variant, NOT transformers' hypothesis heap: every decision stays on the device, so a step is
        one graph.  The W beams of prompt b are rows bW .. bW + W - 1 of an ordinary batched decode step over a cache
        whose rows are copies of the prompt's.  A hypothesis's score is the fp32 sum of its tokens' log-probabilities
        (log-softmax of the step's fp32 logits, no temperature); beam 0 starts at 0 and the others at -inf, so the
        first selection, on the prefill logits, keeps the top W first tokens.  Per step and prompt a live beam offers
        every token, a finished beam (one that took stop_token; None: nothing finishes) only (itself, pad_token) at an
        unchanged score; the best W candidates are kept, best first, exact ties to the lower (beam, token)
        (pg_beam_select), and each row's generated keys and values follow its hypothesis (pg_kv_beam_gather).  The run
        ends when every beam of every prompt is finished (read every check_every steps) or at max_new_tokens.  Final
        score = sum / n ** length_penalty, n = tokens up to and including the stop token (max_new_tokens for an
        unfinished beam); the best num_return_sequences per prompt are returned, best first, ties to the lower beam.
        num_beams = 1 generates exactly generate's greedy ids.

        Returns {"sequences": per prompt a list of id lists, each ending at its stop token; "scores": fp32 [B][R];
        "sum_logprobs": fp32 [B][R]; "beam_rows": int64 [B][R] the final row of each}; with return_trace also "tokens",
        "parents" (int64 [steps][B*W]), "cum" (fp32 [steps][B*W]) and "logits" (a list of fp32 [B*W][V] per step)."""
        w = self.w
        self.beam_args(num_beams, num_return_sequences, max_new_tokens, w.vocab, length_penalty)
        lens_h = mask_lengths(attention_mask)                   # host check, before any launch
        if not 0 <= int(pad_token) < w.vocab or (stop_token is not None and not 0 <= int(stop_token) < w.vocab):
            raise ValueError(f"pad_token {pad_token} / stop_token {stop_token} outside the vocabulary ({w.vocab})")
        if self.tp > 1:
            raise NotImplementedError("generate_beam is not supported under tensor parallelism (tp > 1)")
        B, W, R = input_ids.shape[0], num_beams, num_return_sequences
        rows = B * W
        if rows > ops.BEAM_MAX_ROWS:
            raise ValueError(f"{B} prompts x {W} beams = {rows} rows, more than {ops.BEAM_MAX_ROWS}")
        st, cache, feats, sampler = self.beam_begin(input_ids, pixel_values, attention_mask, max_new_tokens, W,
                                                    stop_token=stop_token, pad_token=pad_token, lens_h=lens_h)
        bm = sampler["beam"]
        trace = {"cum": [bm["cum"].clone()], "logits": [bm["logits"][:, :w.vocab].clone()]} if return_trace else None

        def record():
            if trace is not None:
                trace["logits"].append(bm["logits"][:, :w.vocab].clone())
                trace["cum"].append(bm["cum"].clone())

        n = 1
        step_fn = None
        if use_graph and self.comm.capturable and max_new_tokens > 1:
            step_fn = self._graph_step(st, cache, feats, sampler)
        if step_fn is None:
            step_fn = lambda: self.decode_step(st, cache, feats, sampler)  # noqa: E731
        if check_every is None:
            check_every = 1 if rows == 1 else 8
        while n < max_new_tokens:
            if stop_token is not None and n % check_every == 0 and int(bm["flag"].item()):
                break
            step_fn()
            record()
            n += 1
        hist_tok = st["hist"][:n].cpu()
        hist_par = bm["hist_parent"][:n].cpu().to(torch.int64)
        cum = bm["cum"].cpu()
        self.check_numerics()
        tok_l, par_l = hist_tok.tolist(), hist_par.tolist()
        seqs, scores, sums, brow = [], [], [], []
        for b in range(B):
            hyp = []
            for wi in range(W):
                r = b * W + wi
                toks = self.beam_backtrack(tok_l, par_l, r)
                if stop_token is not None and stop_token in toks:
                    toks = toks[: toks.index(stop_token) + 1]
                    cnt = len(toks)
                else:
                    cnt = max_new_tokens
                c = float(cum[r])
                hyp.append((c / float(cnt) ** float(length_penalty), wi, toks, c))
            # best first; NaN last; ties to the lower beam (a stable sort over beams in order)
            hyp.sort(key=lambda h: (h[0] != h[0], -h[0] if h[0] == h[0] else 0.0))
            seqs.append([h[2] for h in hyp[:R]])
            scores.append([h[0] for h in hyp[:R]])
            sums.append([h[3] for h in hyp[:R]])
            brow.append([b * W + h[1] for h in hyp[:R]])
        out = {"sequences": seqs, "scores": torch.tensor(scores, dtype=torch.float32),
               "sum_logprobs": torch.tensor(sums, dtype=torch.float32), "beam_rows": torch.tensor(brow, dtype=torch.int64)}
        if trace is not None:
            out.update(tokens=hist_tok, parents=hist_par, cum=torch.stack(trace["cum"]).cpu(), logits=trace["logits"])
        return out

    def _graph_step(self, st, cache, feats, sampler):
        """Capture one decode step into a hipGraph (warm-up run first, on a side stream)."""
        torch.cuda.synchronize()
        # warm-up pass to allocate every workspace outside capture, then undo its state advance
        snap = {k: st[k].clone() for k in ("ids", "pos", "kv_len", "step")}
        hist0 = st["hist"].clone()
        res0 = self._ws["d_res_a"][: st["ids"].numel() * self.w.hidden].clone() if st.get("chain") else None
        bm = sampler.get("beam") if sampler is not None else None
        if bm is not None:      # the beam state the warm-up step advances, and the cache window its gather permutes
            bsnap = {k: bm[k].clone() for k in ("cum", "finished", "parent", "hist_parent", "flag")}
            lo, hi = bm["warm_window"]
            kv5 = lambda t: t.view(cache.k.shape[0], cache.B, cache.kv_heads, cache.Smax, -1)  # noqa: E731
            csnap = [(cache.k[:, :, lo:hi], cache.k[:, :, lo:hi].clone()),
                     (cache.vt[..., lo:hi], cache.vt[..., lo:hi].clone()),
                     (kv5(cache.kd)[:, :, :, lo:hi], kv5(cache.kd)[:, :, :, lo:hi].clone()),
                     (kv5(cache.vd)[:, :, :, lo:hi], kv5(cache.vd)[:, :, :, lo:hi].clone())]
        gr = sampler.get("grammar") if sampler is not None else None
        if gr is not None:      # the DFA states the warm-up step moves on: the captured loop must not start a token ahead
            gsnap = {k: gr[k].clone() for k in ("state", "err")}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(s):
                self.decode_step(st, cache, feats, sampler)
            torch.cuda.current_stream().wait_stream(s)
        finally:                                    # restored even when the warm-up step raises
            torch.cuda.synchronize()
            for k, v in snap.items():
                st[k].copy_(v)
            st["hist"].copy_(hist0)
            if res0 is not None:                    # the chained input rows the warm-up step overwrote
                self._ws["d_res_a"][: res0.numel()].copy_(res0)
            if bm is not None:
                for k, v in bsnap.items():
                    bm[k].copy_(v)
                for dst, src in csnap:
                    dst.copy_(src)
            if gr is not None:
                for k, v in gsnap.items():
                    gr[k].copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.decode_step(st, cache, feats, sampler)
        torch.cuda.synchronize()
        self.graphs["decode"] = g
        return g.replay
