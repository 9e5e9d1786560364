// bf16 decode GEMV (M <= 16): gemv_kernel -- the weight ring and the epilogue -- and its launchers (see gemm_common.h);
// the prologues and the 13- / 12-bit block decodes it calls are in gemv_parts.h.
#include "gemv_parts.h"

// --------------------------------------------------------------------------------------
// Skinny GEMM / GEMV (M <= 16): weight streaming straight to VGPRs
// --------------------------------------------------------------------------------------
// One workgroup = 4 waves on NT adjacent 16-row tiles of W (NT = 2 for the interleaved gate/up
// pair); the 4 waves split the chunks of split blockIdx.y round-robin and reduce through LDS.
// Chunk = 32U k: lane (r = lane&15, g = lane>>4) loads 16U contiguous bytes of W row r at
// k = chunk + 8U*g; MFMA step s consumes k = chunk + 8U*g + 8s + [0,8) for BOTH operands, a
// permutation of k that leaves the dot product unchanged.  DEPTH chunks stay in flight in a
// statically indexed register ring.  Plain (temporal) loads: measured 1.2-1.6x faster than
// non-temporal ones on every decode shape (round-1 GEMV sweep).
//
// PRO (prologue, fuses the producer of x into the GEMV so a decode layer needs 5 launches):
//   0: x rows read from A (bf16)
//   1: x = RMSNorm(resid_in + sum_s partials[s]) * (1 + w)       (GemmaRMSNorm, modeling_gemma.py:172-181)
//      workgroup (0,0) also writes resid_out = resid_in + sum partials (ping-pong residual stream)
//   2: x = merge of the split-KV attention partials (2^(m_s - M) weighted, / sum l)
//   3: x = resid * (1 + w), the row's rstd applied in the epilogue;  4: x rows read from A, rstd in the epilogue
// For PRO 1, 2, 3 the WG's K range of x is built in LDS (XPAD, gemv_parts.h); the first weight chunks are issued before
// that prologue.

// tuning knobs (scripts/tune/build_variant.py -D...); every choice that is no longer a knob has its row in DESIGN §A
#ifndef PG_GEMV_D1
#define PG_GEMV_D1 8      // chunks in flight of the one-tile GEMV (M <= 4: batch-1 decode o / down / q|k|v / lm_head)
#endif
#ifndef PG_GEMV_D2
#define PG_GEMV_D2 4      // ... of the two-tile GEMV (M > 4 and the gate/up pair) and of the batched one-tile q|k|v
#endif
#ifndef PG_GEMV_LM_D
#define PG_GEMV_LM_D 6    // ... of the batch-1..4 lm_head GEMV with two 16-row tiles per workgroup (launch_gemv_pro)
#endif
// PG_W_FRAG12 forms that read x straight from memory (down, the finalising down, the lm_head): the ring's first fill
// goes out in two parts.  The first S blocks issue their main and x loads, then the table words (the kernel's oldest
// loads) are waited for and those S blocks' fifth planes follow; every later block of the fill issues its fifth plane
// with its own main loads, as a refill does.  A wide block of the fill then waits for the loads up to its own, not for
// the whole fill (vmcnt retires in order).  0: every fifth plane behind the whole fill (the order before).  Measured
// per kernel with S = 0 / 1 / 2 / 3: down 10.53 / 10.25 / 10.32 / 10.40 us, the lm_head 125.5 / 119.3 /
// 119.7 / -.
#ifndef PG_GEMV_W12_SPLIT
#define PG_GEMV_W12_SPLIT 1
#endif

// CPW > 0: every wave owns exactly CPW chunks (launch checks K / CH / ksplit == 4 * CPW).  The chunk loop is then
// straight-line code with unconditional loads, so hipcc's s_waitcnt bookkeeping stays exact: each chunk's MFMAs
// wait only for that chunk (vmcnt(N), N = younger loads), instead of the conservative vmcnt(0) that the runtime
// loop and its exec-masked loads produce at every ring turn (the ring drained before its first MFMA).
// HOT (PG_KARG_HOT, gemv_hot_kernel): what the loads in front of the weight ring need arrives in SGPRs, the rest of e
// in one batch of scalar loads whose wait must not land in front of the ring -- so PRO 4's sums of squares, which
// only the epilogue consumes and whose addresses need e.f.ss_ld / ss_n, go out right after the ring's first fill
// instead of before it.
template <int EPI, int NT, int U, int DEPTH, int PRO, int FRAG, int CPW = 0, bool HOT = false>
__device__ __forceinline__ void gemv_body(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ W,
                                          int ldw, int K, const EpiArgs& e, const GemvIdx gi) {
  constexpr int CH = U * 32;
  extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int r = lane & 15;
  const int tile0 = gi.bx * NT;
  const int M = e.M;
  const bool xvalid = r < M;

  const int z = gi.by;
  const int nch_all = K / CH;
  const int per_z = (nch_all + gi.ny - 1) / gi.ny;
  const int c0 = z * per_z;
  const int nch = min(nch_all - c0, per_z);
  const int mine = CPW > 0 ? CPW : (nch > wave ? (nch - wave + 3) / 4 : 0);   // chunks wave, wave+4, ...
  // FRAG13: whole blocks (chunk pairs j = 2i, 2i + 1) per wave, the same count for every wave (host-checked)
  constexpr int DB = DEPTH / 2;                 // ... blocks in flight
  const int nb = CPW > 0 ? CPW / 2 : nch >> 3;

  const bf16_t* wrow[NT];
  const bf16_t* wfrag[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int n = (tile0 + t) * 16 + r;
    n = n < e.N ? n : e.N - 1;
    wrow[t] = W + (size_t)n * ldw;
    wfrag[t] = W + (size_t)min(tile0 + t, (e.N >> 4) - 1) * 16 * ldw;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16_t* xs = (bf16_t*)dyn_smem;
  const int Kr = per_z * CH;                    // K range of this split (LDS row length)
  // rows past M read row M-1 (their outputs are never stored): the x loads are unconditional, so the compiler
  // has no select or branch to resolve and no reason to wait for them before issuing the rest of the stream
  const bf16_t* xrow = (PRO == 0 || PRO == 4) ? A + (size_t)(xvalid ? r : M - 1) * lda : nullptr;
  // PRO 4 (M <= 2): wave 0 loads the producer's per-tile sums of squares before the weight stream (all
  // at once, clamped addresses; lanes [32*row, 32*row + 32) own a row) and sums them in the epilogue
  // M > 4 (two tiles per workgroup, <= 64 entries per row): lane (row r, group g) loads entries g + 4k of its
  // own row, so the row total is a reduction over the 4 lane groups
  // (one-tile workgroups at M > 4 -- the batched q|k|v, launch_gemv_pro -- use the same 16-entry layout as the
  // two-tile form)
  constexpr bool SS16 = PRO == 4 && (NT >= 2 || EPI == PG_EPI_QKV_ROPE);
  constexpr int SSL = SS16 ? 16 : 4;
  float ssv[SSL];
#pragma unroll
  for (int k = 0; k < SSL; ++k) ssv[k] = 0.f;
  auto load_ss = [&]() {
    if (wave == 0) {
      if (SS16 && M > 2) {
        const int rr = min(r, M - 1);
#pragma unroll
        for (int k = 0; k < SSL; ++k) ssv[k] = e.f.ss_in[(size_t)rr * e.f.ss_ld + min(g + 4 * k, e.f.ss_n - 1)];
      } else {
        const int lpr = M == 1 ? 64 : 32;
        const int rr = min(lane / lpr, M - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) ssv[k] = e.f.ss_in[(size_t)rr * e.f.ss_ld + min(lane % lpr + k * lpr, e.f.ss_n - 1)];
      }
    }
  };
  if constexpr (PRO == 4 && !HOT) load_ss();
  const bf16_t* xlds = xs + (xvalid ? r : M - 1) * (Kr + XPAD);
  // PG_EPI_QKV_ROPE: the epilogue's rotary positions and cache slot load before the weight stream, its cos/sin
  // right after the first chunks are issued, so the epilogue starts without a dependent round trip
  // (every wave loads them -- a few dwords -- so no divergent branch joins a loaded register, which would make
  // the compiler wait for it right there)
  int rope_p = 0, rope_slot_raw = 0;
  if constexpr (EPI == PG_EPI_QKV_ROPE) {
    rope_p = e.f.pos[r < M ? r : M - 1];
    // a vector load (counted in order with the stream, unlike a scalar load whose wait lands early); a null
    // slot_dev reads a zero word instead of a select on the loaded value
    // (PG_SLOT_ROWS: the word of this lane's row's batch; the same load, issued at the same place)
    const int* slot_p = e.f.slot_dev ? e.f.slot_dev : &pg_zero_word;
    if (e.slot_rows) slot_p += (r < M ? r : M - 1) / e.f.rows_per_batch;
    rope_slot_raw = __hip_atomic_load(slot_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // element offset of a lane's 16-B piece s inside a CH-element chunk: a lane owns 16U contiguous elements.  x uses
  // the same map, so the k order inside the MFMA is consistent.
  constexpr int S_STRIDE = 8;
  const int LANE_OFF = g * 8 * U;
  // The packed layouts' weights are read once, so non-temporal (measured: gate/up 28.7 -> 23.0 us, down 17.0 -> 13.8 us
  // vs row-major plain loads) -- but for q|k|v, whose loads keep the default policy and allocate in the Infinity Cache:
  // the 18 layers' q|k|v (189 MB) then stay on-die across decode steps.
  constexpr bool hot = EPI == PG_EPI_QKV_ROPE;
  auto wload = [&](const auto* p) {
    if constexpr (hot) return *p;
    else return __builtin_nontemporal_load(p);
  };
  u32x4 wb[FRAG >= 2 ? 1 : DEPTH][NT][U];
  u32x4 xb[DEPTH][U];
  W13 wc[FRAG == 2 ? DB : 1][NT];
  // FRAG12: the ring, and the table words (bias | zflag << 8 | wide << 9 | heap slot << 10) of the wave's blocks as
  // scalars -- all CPW / 2 of them in the straight-line forms (tw[t][i]), the ring's in the runtime loop (tw[t][d]).
  // The straight-line forms load them here, ahead of every other load of the kernel: the fifth-plane addresses hang
  // on them, and their round trip then runs beside the prologue's own instead of in front of the stream.
  constexpr int NTW = CPW > 0 ? CPW / 2 : DB;
  W12 wd[FRAG == 3 ? DB : 1][NT];
  unsigned tw[FRAG == 3 ? NT : 1][FRAG == 3 ? NTW : 1];
  unsigned twv[FRAG == 3 && CPW > 0 ? NT : 1][FRAG == 3 && CPW > 0 ? NTW : 1];
  const char* const w12 = (const char*)W;
  const size_t nblk12 = (size_t)(e.N >> 4) * (K >> 7);
  const unsigned* const tab12 = (const unsigned*)(w12 + nblk12 * PG_F12_BLOCK);
  const char* const heap12 = (const char*)tab12 + ((nblk12 * 4 + 255) & ~(size_t)255);
  auto blk12 = [&](int t, int i) {
    return (size_t)min(tile0 + t, (e.N >> 4) - 1) * (K >> 7) + ((c0 >> 3) + i) * 4 + wave;
  };
  if constexpr (FRAG == 3 && CPW > 0) {
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t) twv[t][i] = tab12[blk12(t, i)];
    __builtin_amdgcn_sched_barrier(0);
  }
  // the three planes both packs share, lane-linear: the block's sign/mantissa bytes and its first four code dwords
  auto load_main = [&](const char* p, u32x4 (&sm)[2], u32x4& cq) {
    sm[0] = wload((const u32x4*)p + lane);
    sm[1] = wload((const u32x4*)(p + 1024) + lane);
    cq = wload((const u32x4*)(p + 2048) + lane);
  };
  // block i's twelve main dwords, three lane-linear loads per tile, where the 13-bit ring issues its four
  auto loadm12 = [&](int i, W12 (&wv)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) load_main(w12 + blk12(t, i) * PG_F12_BLOCK, wv[t].sm, wv[t].cq);
  };
  // ... and its fifth plane: the heap line its table word names, unconditionally -- a narrow block names line 0, which
  // every block of the launch shares (cache-hot, no HBM bytes), so there is neither a branch nor a select here.  (A
  // narrow block reading 256 bytes of its own codes instead, to spread the addresses, lost: DESIGN §A.)
  auto load512 = [&](W12 (&wv)[NT], int k) {
    if constexpr (FRAG == 3)
#pragma unroll
      for (int t = 0; t < NT; ++t) wv[t].c5 = ((const unsigned*)(heap12 + (size_t)(tw[t][k] >> 10) * 256))[lane];
  };
  // the runtime loop has no fixed block list to fetch ahead: a block's table word loads with it and its fifth plane
  // waits for that word (this form is the fallback for shapes off the decode's; it is not tuned)
  auto loadw12 = [&](int i, int d, W12 (&wv)[NT]) {
    loadm12(i, wv);
    if constexpr (FRAG == 3)
#pragma unroll
      for (int t = 0; t < NT; ++t) tw[t][d] = __builtin_amdgcn_readfirstlane(tab12[blk12(t, i)]);
    load512(wv, d);
  };
  // block i of this wave: tile t's block (c0 / 8 + i) * 4 + wave, four lane-linear loads and the block's table word
  auto loadw13 = [&](int i, W13 (&wv)[NT]) {
    const int nblk = K >> 7;
    const int bk = ((c0 >> 3) + i) * 4 + wave;
    const char* w13 = (const char*)W;
    const unsigned short* tab = (const unsigned short*)(w13 + (size_t)(e.N >> 4) * nblk * PG_F13_BLOCK);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const size_t blk = (size_t)min(tile0 + t, (e.N >> 4) - 1) * nblk + bk;
      const char* p = w13 + blk * PG_F13_BLOCK;
      load_main(p, wv[t].sm, wv[t].cq);
      wv[t].c4 = wload((const unsigned*)(p + 3072) + lane);
      wv[t].bz = tab[blk];
    }
  };
  // a decoded block's four MFMAs into tile t's accumulator, in the PG_W_FRAG order (chunk, piece)
  auto mfma4 = [&](int t, const u32x4 (&op)[2][2], const u32x4 (&x0)[U], const u32x4 (&x1)[U]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc[t] = mfma16(__builtin_bit_cast(bf16x8, op[h][s]), __builtin_bit_cast(bf16x8, h == 0 ? x0[s] : x1[s]),
                        acc[t]);
  };
  auto mfma12 = [&](const W12 (&wv)[NT], int k, const u32x4 (&x0)[U], const u32x4 (&x1)[U]) {
    static_assert(FRAG != 3 || U == 2, "FRAG12 blocks are two 64-k chunks");
    if constexpr (FRAG == 3)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      u32x4 op[2][2];
      const unsigned w = tw[t][k];
      const unsigned bias = w & 0xffu;
      if (!(w & 0x200u)) decode12<0>(wv[t], bias, op);
      else if (w & 0x100u) decode12<2>(wv[t], bias, op);
      else decode12<1>(wv[t], bias, op);
      mfma4(t, op, x0, x1);
    }
  };
  // block i's 2 x U x NT MFMAs in the PG_W_FRAG order (chunk, piece, tile); the decode is register-only on both sides
  // of its wave-uniform branch
  auto mfma13 = [&](const W13 (&wv)[NT], const u32x4 (&x0)[U], const u32x4 (&x1)[U]) {
    static_assert(FRAG != 2 || U == 2, "FRAG13 blocks are two 64-k chunks");
    // (tile by tile: the tiles' accumulators are independent, each sees its own MFMAs in the PG_W_FRAG order)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      u32x4 op[2][2];
      const unsigned bz = __builtin_amdgcn_readfirstlane(wv[t].bz);
      const unsigned bm = (bz & 0xffu) - 1u;
      if (bz & 0x100u) decode13<true>(wv[t], bm, op);
      else decode13<false>(wv[t], bm, op);
      mfma4(t, op, x0, x1);
    }
  };
  auto loadw = [&](int j, u32x4 (&wv)[NT][U]) {
    if constexpr (FRAG) {
      // fragment-packed weights: tile t's chunk c is U wave-instructions of 1 KiB, lane-linear
      const int cc = c0 + wave + j * 4;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < U; ++s) wv[t][s] = wload((const u32x4*)(wfrag[t] + ((size_t)cc * U + s) * 512 + lane * 8));
    } else {
      const int off = (c0 + wave + j * 4) * CH + LANE_OFF;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < U; ++s) wv[t][s] = *(const u32x4*)(wrow[t] + off + S_STRIDE * s);
    }
  };
  constexpr bool STAGED = PRO != 0 && PRO != 4;   // x built in LDS by a prologue
  auto loadx = [&](int j, u32x4 (&xv)[U]) {
    const int koff = (wave + j * 4) * CH + LANE_OFF;      // offset inside this split
    if constexpr (!STAGED) {
#pragma unroll
      for (int s = 0; s < U; ++s)
        xv[s] = *(const u32x4*)(xrow + c0 * CH + koff + S_STRIDE * s);
    } else {
#pragma unroll
      for (int s = 0; s < U; ++s) xv[s] = *(const u32x4*)(xlds + koff + S_STRIDE * s);
    }
  };
  // The ring of a 13- / 12-bit pack: block i (the chunk pair 2i, 2i + 1) into slot d as a refill issues it, and the
  // MFMAs of the block in slot d
  auto refill_blk = [&](int i, int d) {
    if constexpr (FRAG == 2) {
      loadw13(i, wc[d]);
    } else if constexpr (CPW > 0) {
      loadm12(i, wd[d]);
      load512(wd[d], i);
    } else {
      loadw12(i, d, wd[d]);
    }
    loadx(2 * i, xb[2 * d]);
    loadx(2 * i + 1, xb[2 * d + 1]);
  };
  auto mfma_blk = [&](int i, int d) {
    if constexpr (FRAG == 2) mfma13(wc[d], xb[2 * d], xb[2 * d + 1]);
    else mfma12(wd[d], CPW > 0 ? i : d, xb[2 * d], xb[2 * d + 1]);
  };
  // PRO 1 on one row of at most 2048 elements (batch-1 decode q|k|v): the RMSNorm's loads go out BEFORE the weight ring
  // and are held in registers, so they return first and the normalisation runs while the weights stream (issued after
  // the ring, the prologue's loads made it wait for the whole ring: vmcnt counts in order).  q|k|v only: gate/up too
  // took 152 VGPRs, 3 waves/SIMD, and measured level (profiles/r05_decode_early_prologue_ab.jsonl).
  const bool early = PRO == 1 && EPI == PG_EPI_QKV_ROPE && M == 1 && (K >> 2) <= 512 && e.f.nsplit == 0 &&
                     e.f.resid_out == nullptr;
  Pro1Row p1;
  if constexpr (PRO == 1) {
    if (early) pro1_row_load(e.f, K, p1);
    __builtin_amdgcn_sched_barrier(0);         // (the prologue's loads stay ahead of the ring in the vmcnt order)
  }
  // weights issued before the prologue (its loads are the critical path: the stream overlaps them)
  constexpr bool prew = STAGED;
  if (prew) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if constexpr (FRAG == 2) {
        // (sched_barrier: the blocks' loads stay in ring order, so block 0's MFMAs wait for block 0 alone)
        if (d < DB && d < nb) loadw13(d, wc[d]);
        __builtin_amdgcn_sched_barrier(0);
      } else if constexpr (FRAG == 3) {
        if (d < DB && d < nb) {
          if constexpr (CPW > 0) loadm12(d, wd[d]);
          else loadw12(d, d, wd[d]);
        }
        __builtin_amdgcn_sched_barrier(0);
      } else {
        if (d < mine) loadw(d, wb[d]);
      }
    }
  }
  // FRAG12, straight-line forms: the table words are due (they went out first); the ring's fifth planes follow its main
  // loads, so a narrow block -- whose decode never reads c5 -- still waits for its own twelve dwords alone
  // (the forms without a prologue -- PG_GEMV_W12_SPLIT: only the fill's first S12 blocks take their fifth planes here,
  // behind their own main loads; the fill's later blocks issue theirs with their main loads, the words being scalars by
  // then)
  constexpr int FILL12 = DB < NTW ? DB : NTW;   // blocks of the first fill
  constexpr int S12 = (prew || PG_GEMV_W12_SPLIT <= 0 || PG_GEMV_W12_SPLIT > FILL12) ? FILL12 : PG_GEMV_W12_SPLIT;
  auto fifth12 = [&]() {
    if constexpr (FRAG == 3 && CPW > 0) {
#pragma unroll
      for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) tw[t][i] = __builtin_amdgcn_readfirstlane(twv[t][i]);
#pragma unroll
      for (int d = 0; d < S12; ++d) load512(wd[d], d);
      // (without a prologue behind them nothing that may write memory follows these loads, and the compiler then sinks
      // block 0's into the wide branch of block 0's decode, its only reader: issued there it is the kernel's youngest
      // load, a full round trip behind a vmcnt(0).  The empty statement below may write the heap as far as the compiler
      // knows -- it is handed the pointer, W being __restrict__ -- which pins the loads here; it emits nothing and
      // waits for nothing.)
      if constexpr (!prew) asm volatile("" ::"s"(heap12) : "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  if constexpr (FRAG == 3 && CPW > 0) {
    if (prew) fifth12();
  }
  if constexpr (STAGED) {
    float* scratch = (float*)(dyn_smem + gemv_xs_bytes(M, Kr));
    if (PRO == 1 && early)
      pro1_row_finish(e.f, K, p1, xs, scratch);
    else
      gemv_prologue<PRO>(e, M, K, c0 * CH, nch * CH, xs, scratch, gi);
  }
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if constexpr (FRAG == 2) {
      if (d < DB && d < nb) {
        if (!prew) loadw13(d, wc[d]);
        loadx(2 * d, xb[2 * d]);
        loadx(2 * d + 1, xb[2 * d + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
    } else if constexpr (FRAG == 3) {
      if (d < DB && d < nb) {
        if (!prew) {
          if constexpr (CPW > 0) {
            loadm12(d, wd[d]);
            if (d >= S12) load512(wd[d], d);
          } else {
            loadw12(d, d, wd[d]);
          }
        }
        loadx(2 * d, xb[2 * d]);
        loadx(2 * d + 1, xb[2 * d + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (CPW > 0) {
        if (!prew && d == S12 - 1) fifth12();
      }
    } else if (d < mine) {
      if (!prew) loadw(d, wb[d]);
      loadx(d, xb[d]);
    }
  }
  if constexpr (PRO == 4 && HOT) load_ss();
  // PG_EPI_F32_FIN: the residual rows and norm weights the tile's last-arriving split finalises are loaded now
  // (nothing else writes them in this launch), so the reducer's only round trip is the slab read
  f32x4 fin_r[NT], fin_w[NT];
  i64x2 fin_fa[NT], fin_fb[NT];     // the fixed-point accumulator's entries (PgFusedArgs.fx), converted when used
  if constexpr (EPI == PG_EPI_F32_FIN) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // the lane's own four columns (tile * 16 + q, as the epilogue stores them); a lane past the row's end -- a tile
      // past the last, or the tail of a ragged last tile (N % 16 != 0) -- reads the row's last four, unused
      const int n0 = min((tile0 + t) * 16 + 4 * g, e.N - 4);
      const size_t ro = (size_t)(r < M ? r : M - 1) * e.N + n0;
      // both loads unconditional (a branch or select on them here would make the compiler wait for them before
      // the weight stream): without fx the fixed-point pair reads fin_resid's first 32 bytes, unused; fin_base picks
      fin_r[t] = *(const f32x4*)(e.f.fin_resid + ro);
      const long long* p = e.f.fx ? e.f.fx + ro : (const long long*)e.f.fin_resid;
      fin_fa[t] = *(const i64x2*)p;
      fin_fb[t] = *(const i64x2*)(p + 2);
      // (no select on a loaded value -- it would make the compiler wait right here: a null norm_w reads the
      // residual row instead, unused)
      fin_w[t] = *(const f32x4*)((e.f.norm_w ? e.f.norm_w : e.f.fin_resid) + n0);
    }
  }
  f32x4 rope_cs[NT], rope_sn[NT];
  if constexpr (EPI == PG_EPI_QKV_ROPE) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      bool roped;   // (v columns load a valid, unused entry: no select on the loaded values)
      const int ii = rope_freq_index(e.f, min((tile0 + t) * 16, e.N - 16) + 4 * g, &roped);
      const long off = (long)rope_p * (e.f.head_dim >> 1) + ii;
      rope_cs[t] = *(const f32x4*)(e.f.cos_t + off);
      rope_sn[t] = *(const f32x4*)(e.f.sin_t + off);
    }
  }
  if constexpr (FRAG >= 2 && CPW > 0) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < CPW / 2; ++i) {
      const int d = i % DB;
      mfma_blk(i, d);
      if (i + DB < CPW / 2) refill_blk(i + DB, d);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else if constexpr (FRAG >= 2) {
    for (int base = 0; base < nb; base += DB) {
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const int i = base + d;
        if (i < nb) {
          mfma_blk(i, d);
          if (i + DB < nb) refill_blk(i + DB, d);
        }
      }
    }
  } else if constexpr (CPW > 0) {
    // sched_barrier: the scheduler may not sink the ring's loads below later MFMAs (it otherwise trades the
    // chunks in flight for registers: vmcnt(8) = two chunks in flight on the down projection)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int d = j % DEPTH;
#pragma unroll
      for (int s = 0; s < U; ++s) {
        const bf16x8 xv = __builtin_bit_cast(bf16x8, xb[d][s]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma16(__builtin_bit_cast(bf16x8, wb[d][t][s]), xv, acc[t]);
      }
      if (j + DEPTH < CPW) {
        loadw(j + DEPTH, wb[d]);
        loadx(j + DEPTH, xb[d]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    for (int base = 0; base < mine; base += DEPTH) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) {
        const int j = base + d;
        if (j < mine) {
#pragma unroll
          for (int s = 0; s < U; ++s) {
            const bf16x8 xv = __builtin_bit_cast(bf16x8, xb[d][s]);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma16(__builtin_bit_cast(bf16x8, wb[d][t][s]), xv, acc[t]);
          }
          if (j + DEPTH < mine) {
            loadw(j + DEPTH, wb[d]);
            loadx(j + DEPTH, xb[d]);
          }
        }
      }
    }
  }

  __shared__ f32x4 red[4][NT][64];
#pragma unroll
  for (int t = 0; t < NT; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  // PgFusedArgs.amax_zero (ABI 12 for this kernel): workgroup (0, 0) clears amax_zero[0 .. n) after its stream -- the
  // batch-1 decode step's first GEMV zeroes the fixed-point accumulator that the step's FX_ADD producers add into,
  // so no state carries over from an interrupted step (n % 4 == 0, 16-B aligned, host-checked)
  if (e.f.amax_zero && gi.bx == 0 && gi.by == 0)
    for (int i = 4 * (int)threadIdx.x; i < e.f.amax_zero_n; i += 1024) *(u32x4*)(e.f.amax_zero + i) = u32x4{0u, 0u, 0u, 0u};
  if (wave != 0) return;
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = red[0][t][lane] + red[1][t][lane] + red[2][t][lane] + red[3][t][lane];
  // lane holds C[m = lane&15][n = tile*16 + 4*(lane>>4) + 0..3]
  const int m = r;
  const int q = 4 * g;
  if constexpr (PRO == 3) {
    const float* scratch = (const float*)(dyn_smem + gemv_xs_bytes(M, Kr));
    const float rs = scratch[64 + (m < M ? m : 0)];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] *= rs;
  }
  if constexpr (PRO == 4) {
    // the raw per-tile entries were loaded with clamped indices (no select before the weight stream): mask here
    float ss = 0.f;
    if (SS16 && M > 2) {
#pragma unroll
      for (int k = 0; k < SSL; ++k) ss += g + 4 * k < e.f.ss_n ? ssv[k] : 0.f;
    } else {
      const int lpr = M == 1 ? 64 : 32;
#pragma unroll
      for (int k = 0; k < 4; ++k) ss += lane % lpr + k * lpr < e.f.ss_n ? ssv[k] : 0.f;
    }
    if (SS16 && M > 2) {
      ss = sum_xor16(ss);
      ss = sum_xor32(ss);
    } else {
      const int lpr = M == 1 ? 64 : 32;
      for (int o = 1; o < lpr; o <<= 1) ss += __shfl_xor(ss, o, 64);
      ss = __shfl(ss, (m < M ? m : 0) * lpr, 64);
    }
    const float rs = rsqrtf(ss / (float)K + e.f.eps);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] *= rs;
  }
  if constexpr (EPI == PG_EPI_F32_FIN) {
    // 1. this split's slab; 2. release + ticket; 3. the last split of the tile reduces the slabs into the
    //    residual rows it owns and writes their sum of squares (MI355X guide: in-launch split-K reduction)
    // Slab stores are write-through (agent-scope relaxed 8-B atomic stores = global_store sc1), drained,
    // then one relaxed agent ticket: no release fence (an L2 write-back per workgroup cost 2x the kernel).
    // The reducer reads the slabs with sc1 loads (bypass its L1/L2), so no acquire fence either.
    const PgFusedArgs& f = e.f;
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    // one sum-of-squares entry per tile pair (per tile at NT 1): a 4-tile workgroup writes two
    constexpr int SE = NT >= 2 ? NT / 2 : 1;
    auto finish = [&](int t, int n0, f32x4 v, float& ssl) {   // v = the finalised residual of (m, n0..n0+3)
      *(f32x4*)(f.fin_resid + (size_t)m * e.N + n0) = v;
      ssl += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      if (f.fin_x) {
        const f32x4 w = fin_w[t];
        u32x2 pk;
        pk[0] = pack_bf2(v[0] * (1.0f + w[0]), v[1] * (1.0f + w[1]));
        pk[1] = pack_bf2(v[2] * (1.0f + w[2]), v[3] * (1.0f + w[3]));
        *(u32x2*)(f.fin_x + (size_t)m * e.N + n0) = pk;
      }
    };
    // the residual entering the finalisation: fin_resid, or with fx the fixed-point accumulator, which then holds the
    // whole residual (its entries are cleared by this tile's finalising workgroup: every split of the tile loaded
    // them before its ticket)
    auto fin_base = [&](int t) {
      return f.fx ? f32x4{fx_to_f32(fin_fa[t][0]), fx_to_f32(fin_fa[t][1]), fx_to_f32(fin_fb[t][0]),
                          fx_to_f32(fin_fb[t][1])}
                  : fin_r[t];
    };
    auto fx_clear = [&](int n0) {
      if (f.fx) {
        long long* p = f.fx + (size_t)m * e.N + n0;
        *(i64x2*)p = i64x2{0, 0};
        *(i64x2*)(p + 2) = i64x2{0, 0};
      }
    };
    auto put_ss = [&](float (&ssl)[SE]) {
#pragma unroll
      for (int p = 0; p < SE; ++p) {
        const float v = sum_xor32(sum_xor16(ssl[p]));
        if (g == 0 && m < M) f.ss_out[(size_t)m * f.ss_ld + gi.bx * SE + p] = v;
      }
    };
    if (gi.ny == 1) {
      // no split: this workgroup owns the tile -- no slab, no ticket (same sums: residual + (acc + bias))
      float ssl[SE];
#pragma unroll
      for (int p = 0; p < SE; ++p) ssl[p] = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n0 = (tile0 + t) * 16 + q;
        if (m < M && n0 < e.N) {
          f32x4 v = acc[t];
          if (e.bias) v += load4_guard(e.bias, n0, e.N);
          finish(t, n0, fin_base(t) + v, ssl[t / 2 < SE ? t / 2 : 0]);
          fx_clear(n0);
        }
      }
      put_ss(ssl);
      return;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n0 = (tile0 + t) * 16 + q;
      if (m < M && n0 < e.N) {
        f32x4 v = acc[t];
        if (e.bias && z == 0) v += load4_guard(e.bias, n0, e.N);
        gu64* dst = (gu64*)((float*)e.C + ((size_t)z * M + m) * e.ldc + n0);
        __hip_atomic_store(dst, __builtin_bit_cast(unsigned long long, u32x2{__float_as_uint(v[0]),
                           __float_as_uint(v[1])}), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dst + 1, __builtin_bit_cast(unsigned long long, u32x2{__float_as_uint(v[2]),
                           __float_as_uint(v[3])}), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(f.fin_cnt + gi.bx, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0, 64);
    if (old != gi.ny - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // compiler-only: keep the loads below the ticket
    float ssl[SE];
#pragma unroll
    for (int p = 0; p < SE; ++p) ssl[p] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n0 = (tile0 + t) * 16 + q;
      if (m < M && n0 < e.N) {
        f32x4 v = fin_base(t);
        // all (<= 8) slabs in flight at once: clamped addresses + selects, no per-split branch / wait
        const int Z = gi.ny;
        u32x2 sa[8], sb[8];
#pragma unroll
        for (int zz = 0; zz < 8; ++zz) {
          gu64* src = (gu64*)((float*)e.C + ((size_t)(zz < Z ? zz : Z - 1) * M + m) * e.ldc + n0);
          sa[zz] = __builtin_bit_cast(u32x2, __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          sb[zz] = __builtin_bit_cast(u32x2, __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
#pragma unroll
        for (int zz = 0; zz < 8; ++zz) {
          const f32x4 sv = {__uint_as_float(sa[zz][0]), __uint_as_float(sa[zz][1]), __uint_as_float(sb[zz][0]),
                            __uint_as_float(sb[zz][1])};
          v += zz < Z ? sv : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        finish(t, n0, v, ssl[t / 2 < SE ? t / 2 : 0]);
        fx_clear(n0);
      }
    }
    put_ss(ssl);
    if (lane == 0) __hip_atomic_store(f.fin_cnt + gi.bx, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if constexpr (EPI == PG_EPI_F32_ADD) {
    // C[m][n] += acc (+ bias by split 0): hardware float atomic adds at the memory side, no slab, no ticket --
    // the launch ends one atomic round trip after its last MFMA (the F32_FIN tail is slab store -> ticket -> slab
    // load).  The split order of the adds is unordered (fp32 rounding of the sum may differ run to run).
    if (m < M) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n0 = (tile0 + t) * 16 + q;
        if (n0 < e.N) {
          f32x4 v = acc[t];
          if (e.bias && z == 0) v += load4_guard(e.bias, n0, e.N);
          float* dst = (float*)e.C + (size_t)m * e.ldc + n0;
#pragma unroll
          for (int j = 0; j < 4; ++j) unsafeAtomicAdd(dst + j, v[j]);
        }
      }
    }
    return;
  }
  if constexpr (EPI == PG_EPI_FX_ADD) {
    // C[m][n] += rn(acc * 2^32) by 64-bit integer atomics (global_atomic_add_u64 at the memory side): the same one
    // round trip after the last MFMA as F32_ADD, but integer addition is associative, so the accumulated sum --
    // and every residual read from it -- is the same bits whatever order the splits arrive in
    if (m < M) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n0 = (tile0 + t) * 16 + q;
        if (n0 < e.N) {
          f32x4 v = acc[t];
          if (e.bias && z == 0) v += load4_guard(e.bias, n0, e.N);
          // resid_in (optional): split 0 also adds the fp32 residual rows -- the accumulator then holds the whole
          // residual, and its consumers read it alone
          if (e.f.resid_in && z == 0) v += load4_guard(e.f.resid_in + (size_t)m * e.N, n0, e.N);
          unsigned long long* dst = (unsigned long long*)e.C + (size_t)m * e.ldc + n0;
#pragma unroll
          for (int j = 0; j < 4; ++j) atomicAdd(dst + j, (unsigned long long)fx_from_f32_checked(v[j], e.f.status));
        }
      }
    }
    return;
  }
  if constexpr (EPI == PG_EPI_BF16_GELU_MUL) {
#pragma unroll
    for (int t = 0; t < NT; t += 2) epi_gelu_mul4(e, m, (tile0 + t) * 16, q, acc[t], acc[t + 1]);
  } else if constexpr (EPI == PG_EPI_QKV_ROPE) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 v = acc[t];
      const int n0 = (tile0 + t) * 16 + q;
      if (e.bias && n0 < e.N) v += load4_guard(e.bias, n0, e.N);
      f32x4 pr;
#pragma unroll
      for (int j = 0; j < 4; ++j) pr[j] = xchg_xor32(v[j]);
      epi_qkv_rope4_core(e, m, n0, v, pr, rope_cs[t], rope_sn[t], e.f.slot_base + rope_slot_raw);
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) epi_store4<EPI>(e, m, (tile0 + t) * 16 + q, acc[t], z);
  }
}

// (the 13-bit gate/up GEMV is held to 4 waves per SIMD, its PG_W_FRAG twin's occupancy: left alone the allocator takes
// 122 VGPRs + 12 AGPRs, three waves; told, it fits 128 without a spill)
template <int EPI, int NT, int U, int DEPTH, int PRO, int FRAG, int CPW = 0>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(FRAG >= 2 && CPW > 0 && EPI == PG_EPI_BF16_GELU_MUL ? 4 : 1, 8)))
void gemv_kernel(EpiArgs e, const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ W, int ldw, int K) {
  gemv_body<EPI, NT, U, DEPTH, PRO, FRAG, CPW>(A, lda, W, ldw, K, e,
                                               GemvIdx{(int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y});
}

// PG_KARG_HOT: the batch-1 decode forms on the exponent-coded packs that gain from it (gate/up, down, the finalising
// down, the lm_head: launch_gemv13) take a hot argument header, 14 dwords, 8-byte fields first so that no padding counts
// against the preload: W, three pointers and a 64-bit word whose meaning the form fixes, N, K, mf = M | gridDim.y << 16
// (the K split count, which the kernel otherwise reads from the dispatch's hidden arguments in front of everything
// else), ldw.  In order of first use:
//   PRO 1:     h0 = fx, h1 = resid_in, h2 = norm_w
//   PRO 0 / 4: h0 = A, h2 = ss_in, x3 = lda
// The header's fields overwrite their twins in a copy of e (registers: the copy is split field by field), so the body
// reads one EpiArgs whichever signature brought it.  (gemv_kernel above takes its struct FIRST for the same reason
// turned round: the preload stops at the first aggregate, so the forms that keep that signature -- q|k|v, which lost
// 0.3 us a launch on a header, o_proj, which gained nothing, and every batched one -- run the entry code they had
// before this source was compiled with the preload)
template <int EPI, int NT, int U, int DEPTH, int PRO, int FRAG, int CPW = 0>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(FRAG >= 2 && CPW > 0 && EPI == PG_EPI_BF16_GELU_MUL ? 4 : 1, 8)))
void gemv_hot_kernel(const bf16_t* __restrict__ W, const void* h0, const void* h1, const void* h2,
                     unsigned long long x3, int N, int K, int mf, int ldw, const bf16_t* __restrict__ A, int lda,
                     EpiArgs e) {
  static_assert(PRO == 0 || PRO == 1 || PRO == 4, "forms with a header");
  EpiArgs eh = e;
  eh.N = N;
  eh.M = mf & 0xffff;
  if constexpr (PRO == 1) {
    eh.f.fx = (long long*)h0;
    eh.f.resid_in = (const float*)h1;
    eh.f.norm_w = (const float*)h2;
  } else {
    A = (const bf16_t*)h0;
    lda = (int)x3;
    eh.f.ss_in = (const float*)h2;
  }
  gemv_body<EPI, NT, U, DEPTH, PRO, FRAG, CPW, true>(
      A, lda, W, ldw, K, eh, GemvIdx{(int)blockIdx.x, (int)blockIdx.y, 0, (int)((unsigned)mf >> 16)});
}

// one launch of a gemv_kernel instantiation: HOT (and PG_KARG_HOT) fills the header from the same EpiArgs
template <bool HOT, int EPI, int NT, int DEPTH, int PRO, int FRAG, int CPW>
static void launch_gemv_one(dim3 grid, size_t lds, hipStream_t st, const bf16_t* A, int lda, const bf16_t* W, int ldw,
                            int K, const EpiArgs& e) {
  if constexpr (HOT && PG_KARG_HOT) {
    const PgFusedArgs& f = e.f;
    const void *h0 = nullptr, *h1 = nullptr, *h2 = nullptr;
    unsigned long long x3 = 0;
    if (PRO == 1) h0 = f.fx, h1 = f.resid_in, h2 = f.norm_w;
    else h0 = A, h2 = f.ss_in, x3 = (unsigned)lda;
    hipLaunchKernelGGL((gemv_hot_kernel<EPI, NT, 2, DEPTH, PRO, FRAG, CPW>), grid, dim3(256), lds, st, W, h0, h1, h2, x3,
                       e.N, K, (int)(e.M | grid.y << 16), ldw, A, lda, e);
  } else {
    hipLaunchKernelGGL((gemv_kernel<EPI, NT, 2, DEPTH, PRO, FRAG, CPW>), grid, dim3(256), lds, st, e, A, lda, W, ldw, K);
  }
}

// One launch with the chunks-per-wave specialisation (see gemv_body) when every wave owns cpw chunks -- 4, 8 or, with
// C16, 16 of them -- and the runtime chunk loop otherwise.
template <bool HOT, bool C16, int EPI, int NT, int DEPTH, int PRO, int FRAG>
static void launch_gemv_cpw(int cpw, dim3 grid, size_t lds, hipStream_t st, const bf16_t* A, int lda, const bf16_t* W,
                            int ldw, int K, const EpiArgs& e) {
  switch (cpw) {
    case 4: launch_gemv_one<HOT, EPI, NT, DEPTH, PRO, FRAG, 4>(grid, lds, st, A, lda, W, ldw, K, e); return;
    case 8: launch_gemv_one<HOT, EPI, NT, DEPTH, PRO, FRAG, 8>(grid, lds, st, A, lda, W, ldw, K, e); return;
    case 16:
      if constexpr (C16) {
        launch_gemv_one<HOT, EPI, NT, DEPTH, PRO, FRAG, 16>(grid, lds, st, A, lda, W, ldw, K, e);
        return;
      }
      [[fallthrough]];
    default: launch_gemv_one<HOT, EPI, NT, DEPTH, PRO, FRAG, 0>(grid, lds, st, A, lda, W, ldw, K, e);
  }
}

// bf16 weights, row-major or PG_W_FRAG: NT tiles per workgroup and DEPTH chunks in flight (U = 2: 64-element chunks),
// the chunks-per-wave specialisation when the K split is exact
template <int EPI, int NT, int DEPTH, int PRO, bool FRAG>
static void launch_gemv_tiles(const bf16_t* A, int lda, const bf16_t* W, int ldw, int K, int ksplit, const EpiArgs& e,
                              hipStream_t st) {
  const int ntiles = (e.N + 15) / 16, nch = K / 64;
  const size_t lds = gemv_lds_bytes(PRO, e.M, (nch + ksplit - 1) / ksplit * 64);
  const int cpw = (nch % ksplit == 0 && (nch / ksplit) % 4 == 0) ? nch / ksplit / 4 : 0;
  launch_gemv_cpw<false, true, EPI, NT, DEPTH, PRO, FRAG>(cpw, dim3((ntiles + NT - 1) / NT, ksplit), lds, st, A, lda, W,
                                                          ldw, K, e);
}

// measured configs (round-1 GEMV sweep): M <= 4: one tile per WG, U=2, 8 chunks in flight;
// M > 4 and the gate/up pair: two tiles per WG, U=2, 4 chunks in flight.
// ring depths re-checked on the final round-2 code: two-tile kernels 4 chunks in flight, one-tile 8
template <int EPI, int PRO, bool FRAG>
static void launch_gemv_pro(const bf16_t* A, int lda, const bf16_t* W, int ldw, int K, int ksplit, const EpiArgs& e,
                            hipStream_t st) {
  if constexpr (EPI == PG_EPI_QKV_ROPE) {
    // batched q|k|v (2560 rows): one tile per workgroup doubles the grid to 160 workgroups
    if (e.M > 4) return launch_gemv_tiles<EPI, 1, PG_GEMV_D2, PRO, FRAG>(A, lda, W, ldw, K, ksplit, e, st);
  }
  if constexpr (EPI == PG_EPI_F32) {
    // the lm_head at batch 1-4 with two tiles per workgroup (one tile: +5.5 us per token at 6 chunks in flight, +3.5
    // at 4: profiles/r05_lm_head_nt2_ab.jsonl)
    if (e.M <= 4 && (e.N + 15) / 16 >= 8192 && ksplit == 1)
      return launch_gemv_tiles<EPI, 2, PG_GEMV_LM_D, PRO, FRAG>(A, lda, W, ldw, K, 1, e, st);
  }
  // Two tiles per workgroup for the gate/up pair and at 5..16 rows, one tile for the rest.  (Four tiles at 5..16 rows
  // -- x's share of a workgroup's bytes 1/5 instead of 1/3 -- measured slower on the pt-448 x16 gate/up and finalised
  // down: 1.408 vs 1.380 ms/step; the epilogues take any even NT.  Round 5: two gate/up pairs per workgroup at batch 1
  // -- half the workgroups re-reading the row -- measured slower, 1.061 vs 1.059 ms/token at 3 chunks in flight, 1.073
  // at 2: profiles/r05_gateup_nt4_ab.jsonl)
  if (EPI == PG_EPI_BF16_GELU_MUL || e.M > 4)
    launch_gemv_tiles<EPI, 2, PG_GEMV_D2, PRO, FRAG>(A, lda, W, ldw, K, ksplit, e, st);
  else
    launch_gemv_tiles<EPI, 1, PG_GEMV_D1, PRO, FRAG>(A, lda, W, ldw, K, ksplit, e, st);
}


template <int EPI, bool FRAG>
static void launch_gemv(const bf16_t* A, int lda, const bf16_t* W, int ldw, int K, int ksplit, const EpiArgs& e,
                        hipStream_t st) {
  if constexpr (EPI == PG_EPI_F32_ADD || EPI == PG_EPI_FX_ADD) {   // (plain x, or the attention merge: o / down)
    if (e.f.pro_mode == 2)
      launch_gemv_pro<EPI, 2, FRAG>(A, lda, W, ldw, K, ksplit, e, st);
    else
      launch_gemv_pro<EPI, 0, FRAG>(A, lda, W, ldw, K, ksplit, e, st);
    return;
  }
  switch (e.f.pro_mode) {
    case 1: launch_gemv_pro<EPI, 1, FRAG>(A, lda, W, ldw, K, ksplit, e, st); break;
    case 2: launch_gemv_pro<EPI, 2, FRAG>(A, lda, W, ldw, K, ksplit, e, st); break;
    case 3: launch_gemv_pro<EPI, 3, FRAG>(A, lda, W, ldw, K, ksplit, e, st); break;
    case 4: launch_gemv_pro<EPI, 4, FRAG>(A, lda, W, ldw, K, ksplit, e, st); break;
    default: launch_gemv_pro<EPI, 0, FRAG>(A, lda, W, ldw, K, ksplit, e, st); break;
  }
}

// PG_W_FRAG13 / PG_W_FRAG12 (F = 2 / 3): the batch-1 decode forms, each with the depth and tile count of its PG_W_FRAG
// twin (launch_gemv_pro at M <= 4) -- here the two-tile lm_head form takes every N.  CPW 4 and 8 are the chunk counts
// the decode shapes hit.
template <int EPI, int NT, int DEPTH, int PRO, int F>
static void launch_gemv13(const bf16_t* A, int lda, const void* W, int K, int ksplit, const EpiArgs& e, hipStream_t st) {
  static_assert(DEPTH % 2 == 0, "whole blocks in flight");
  const int ntiles = e.N / 16;
  const int per_z = K / 64 / ksplit;
  // the hot argument header for the forms it gained on; q|k|v and o_proj keep the struct (§A)
  constexpr bool HOT = PRO == 0 || PRO == 4 || EPI == PG_EPI_BF16_GELU_MUL;
  launch_gemv_cpw<HOT, false, EPI, NT, DEPTH, PRO, F>(per_z / 4, dim3((ntiles + NT - 1) / NT, ksplit),
                                                      gemv_lds_bytes(PRO, e.M, per_z * 64), st, A, lda,
                                                      (const bf16_t*)W, K, K, e);
}

template <int F>
static int dispatch_gemv13(int epi, const bf16_t* A, int lda, const void* W, int K, int ksplit, const EpiArgs& e,
                           hipStream_t st) {
  const int pm = e.f.pro_mode;
  if (e.M > 4 || (K / 64) % (8 * ksplit)) return (int)hipErrorInvalidValue;
  if (epi == PG_EPI_QKV_ROPE && pm == 1) launch_gemv13<PG_EPI_QKV_ROPE, 1, PG_GEMV_D1, 1, F>(A, lda, W, K, ksplit, e, st);
  else if (epi == PG_EPI_FX_ADD && pm == 2) launch_gemv13<PG_EPI_FX_ADD, 1, PG_GEMV_D1, 2, F>(A, lda, W, K, ksplit, e, st);
  else if (epi == PG_EPI_FX_ADD && pm == 0) launch_gemv13<PG_EPI_FX_ADD, 1, PG_GEMV_D1, 0, F>(A, lda, W, K, ksplit, e, st);
  else if (epi == PG_EPI_F32_FIN && pm == 0) launch_gemv13<PG_EPI_F32_FIN, 1, PG_GEMV_D1, 0, F>(A, lda, W, K, ksplit, e, st);
  else if (epi == PG_EPI_BF16_GELU_MUL && pm == 1)
    launch_gemv13<PG_EPI_BF16_GELU_MUL, 2, PG_GEMV_D2, 1, F>(A, lda, W, K, ksplit, e, st);
  else if (epi == PG_EPI_F32 && pm == 4) launch_gemv13<PG_EPI_F32, 2, PG_GEMV_LM_D, 4, F>(A, lda, W, K, ksplit, e, st);
  else return (int)hipErrorInvalidValue;
  return 0;
}

int pg_dispatch_gemv13(int epi, int bits, const bf16_t* A, int lda, const void* W, int K, int ksplit, const EpiArgs& e,
                       hipStream_t st) {
  return bits == 12 ? dispatch_gemv13<3>(epi, A, lda, W, K, ksplit, e, st)
                    : dispatch_gemv13<2>(epi, A, lda, W, K, ksplit, e, st);
}

int pg_dispatch_gemv(int epi, bool frag, const bf16_t* A, int lda, const bf16_t* W, int ldw, int K, int ksplit,
                     const EpiArgs& e, hipStream_t st) {
#define PG_CASE(E)                                                                             \
  case E:                                                                                      \
    if (frag) launch_gemv<E, true>(A, lda, W, ldw, K, ksplit, e, st);                          \
    else launch_gemv<E, false>(A, lda, W, ldw, K, ksplit, e, st);                              \
    return 0;
#define PG_CASE_ROWMAJOR(E)                                                                    \
  case E: launch_gemv<E, false>(A, lda, W, ldw, K, ksplit, e, st); return 0;
  switch (epi) {
    PG_CASE(PG_EPI_BF16)
    PG_CASE(PG_EPI_BF16_GELU_MUL)
    PG_CASE(PG_EPI_F32)
    PG_CASE(PG_EPI_QKV_ROPE)
    PG_CASE(PG_EPI_F32_FIN)
    PG_CASE(PG_EPI_F32_ADD)
    PG_CASE(PG_EPI_FX_ADD)
    PG_CASE_ROWMAJOR(PG_EPI_BF16_GELU)
    PG_CASE_ROWMAJOR(PG_EPI_F32_POS)
    PG_CASE_ROWMAJOR(PG_EPI_BF16_VT)
    default: return (int)hipErrorInvalidValue;
  }
#undef PG_CASE
#undef PG_CASE_ROWMAJOR
}
