// Parts of the bf16 decode GEMV that gemv_body (gemm_gemv.hip) only calls: the LDS-only barrier, the prologues that
// build x in LDS, and the 13- / 12-bit weight blocks with their decodes.
#pragma once
#include "gemm_common.h"

// For PRO != 0 the WG's K range of x is built in LDS (bf16, rows padded by 16 B against bank conflicts).
#define XPAD 8

// the GEMV's workgroup coordinates (blockIdx / gridDim of its launch)
struct GemvIdx {
  int bx, by, nx, ny;
};

// bytes of the x image a prologue stages in LDS, M rows of Kr (+ pad) bf16: the prologue's scratch floats start here
__host__ __device__ constexpr size_t gemv_xs_bytes(int M, int Kr) {
  return ((size_t)M * (Kr + XPAD) * 2 + 15) & ~(size_t)15;
}
// LDS of a launch whose split covers Kr elements of x: the staged image (PRO 1, 2, 3) and the prologue's scratch
__host__ __device__ constexpr size_t gemv_lds_bytes(int PRO, int M, int Kr) {
  if (PRO == 0 || PRO == 4) return 0;
  return gemv_xs_bytes(M, Kr) + (PRO == 1 ? 64 : PRO == 3 ? 80 : 0) * sizeof(float);
}

// A workgroup barrier that orders LDS only: the wave's LDS ops are waited for, its global loads (the weight ring) stay
// in flight (__syncthreads' fence would wait for them too: s_waitcnt vmcnt(0))
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}
// The batch-1 RMSNorm prologue in two halves (PRO 1, M == 1, K <= 2048): the loads -- thread t owns the float4s
// c = t and t + 256 of the row, the residual's and the norm weight's, the fixed-point accumulator's raw words --
// and, after the weight ring is issued, the sum of squares, the normalisation and the LDS image.
struct Pro1Row {
  f32x4 a[2], w[2];
  i64x2 qa[2], qb[2];
};
__device__ __forceinline__ void pro1_row_load(const PgFusedArgs& f, int K, Pro1Row& p) {
  const int t = threadIdx.x, K4 = K >> 2;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = t + i * 256;
    p.a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    p.w[i] = p.a[i];
    p.qa[i] = i64x2{0, 0};
    p.qb[i] = p.qa[i];
    if (c < K4) {
      p.w[i] = ((const f32x4*)f.norm_w)[c];
      if (f.resid_in) p.a[i] = ((const f32x4*)f.resid_in)[c];
      if (f.fx) {
        p.qa[i] = *(const i64x2*)(f.fx + 4 * c);
        p.qb[i] = *(const i64x2*)(f.fx + 4 * c + 2);
      }
    }
  }
}
__device__ __forceinline__ void pro1_row_finish(const PgFusedArgs& f, int K, const Pro1Row& p, bf16_t* xs,
                                                float* red) {
  const int t = threadIdx.x, K4 = K >> 2;
  f32x4 v[2];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    v[i] = p.a[i];
    if (f.fx) v[i] += f32x4{fx_to_f32(p.qa[i][0]), fx_to_f32(p.qa[i][1]), fx_to_f32(p.qb[i][0]), fx_to_f32(p.qb[i][1])};
    ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
  }
  ss = wave_sum(ss);
  if ((t & 63) == 0) red[t >> 6] = ss;
  lds_barrier();
  const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + f.eps);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = t + i * 256;
    if (c < K4) {
      const f32x4 w = p.w[i];
      u32x2 pk;
      pk[0] = pack_bf2((v[i][0] * rstd) * (1.0f + w[0]), (v[i][1] * rstd) * (1.0f + w[1]));
      pk[1] = pack_bf2((v[i][2] * rstd) * (1.0f + w[2]), (v[i][3] * rstd) * (1.0f + w[3]));
      *(u32x2*)(xs + c * 4) = pk;
    }
  }
  lds_barrier();
}

template <int PRO>
__device__ __forceinline__ void gemv_prologue(const EpiArgs& e, int M, int K, int k0, int Kr, bf16_t* xs,
                                              float* scratch, const GemvIdx& gi) {
  const PgFusedArgs& f = e.f;
  const int t = threadIdx.x;
  const int ldx = Kr + XPAD;
  if constexpr (PRO == 1) {
    // RMSNorm over the FULL row (Kr == K): pass 1 sum of squares, pass 2 normalise into LDS
    const int K4 = K >> 2;
    const bool w0 = gi.bx == 0 && gi.by == 0 && f.resid_out != nullptr;
    float* red = scratch;   // [4 waves][16 rows]
    if (M == 1 && K4 <= 4 * 256) {
      // one row: keep it in registers between the two passes (one dependent round trip fewer)
      f32x4 v[4], wn[4];
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = t + i * 256;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < K4) {
          wn[i] = ((const f32x4*)f.norm_w)[c];          // issued with the residual: one round trip
          f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
          if (f.resid_in) a = ((const f32x4*)f.resid_in)[c];
          if (f.fx) a += fx_load4(f.fx + 4 * c);
          for (int sp = 0; sp < f.nsplit; ++sp) a += ((const f32x4*)(f.partials + (size_t)sp * K))[c];
          v[i] = a;
          ss += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3];
          if (w0) ((f32x4*)f.resid_out)[c] = a;
        }
      }
      ss = wave_sum(ss);
      if ((t & 63) == 0) red[t >> 6] = ss;
      __syncthreads();
      const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + f.eps);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = t + i * 256;
        if (c < K4) {
          const f32x4 w = wn[i];
          u32x2 pk;
          pk[0] = pack_bf2((v[i][0] * rstd) * (1.0f + w[0]), (v[i][1] * rstd) * (1.0f + w[1]));
          pk[1] = pack_bf2((v[i][2] * rstd) * (1.0f + w[2]), (v[i][3] * rstd) * (1.0f + w[3]));
          *(u32x2*)(xs + c * 4) = pk;
        }
      }
      __syncthreads();
      return;
    }
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
      for (int c = t; c < K4; c += 256) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (f.resid_in) v = ((const f32x4*)(f.resid_in + (size_t)m * K))[c];
        if (f.fx) v += fx_load4(f.fx + (size_t)m * K + 4 * c);
        for (int sp = 0; sp < f.nsplit; ++sp) v += ((const f32x4*)(f.partials + ((size_t)sp * M + m) * K))[c];
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        if (w0) ((f32x4*)(f.resid_out + (size_t)m * K))[c] = v;
      }
      ss = wave_sum(ss);
      if ((t & 63) == 0) red[(t >> 6) * 16 + m] = ss;
    }
    __syncthreads();
    for (int m = 0; m < M; ++m) {
      const float rstd = rsqrtf((red[m] + red[16 + m] + red[32 + m] + red[48 + m]) / (float)K + f.eps);
      for (int c = t; c < K4; c += 256) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (f.resid_in) v = ((const f32x4*)(f.resid_in + (size_t)m * K))[c];
        if (f.fx) v += fx_load4(f.fx + (size_t)m * K + 4 * c);
        for (int sp = 0; sp < f.nsplit; ++sp) v += ((const f32x4*)(f.partials + ((size_t)sp * M + m) * K))[c];
        const f32x4 w = ((const f32x4*)f.norm_w)[c];
        u32x2 pk;
        pk[0] = pack_bf2((v[0] * rstd) * (1.0f + w[0]), (v[1] * rstd) * (1.0f + w[1]));
        pk[1] = pack_bf2((v[2] * rstd) * (1.0f + w[2]), (v[3] * rstd) * (1.0f + w[3]));
        *(u32x2*)(xs + m * ldx + c * 4) = pk;
      }
    }
  } else if constexpr (PRO == 3) {
    // x = resid * (1 + w) over the full row (the residual was finalised by the producer's FIN epilogue);
    // per-row rstd from the producer's per-tile sums of squares, applied in the epilogue (scratch[64 + m])
    const int K4 = K >> 2;
    float* red = scratch;   // [4 waves][16 rows], then rstd [16] at +64
    for (int m = 0; m < M; ++m) {
      for (int c = t; c < K4; c += 256) {
        const f32x4 v = ((const f32x4*)(f.resid_in + (size_t)m * K))[c];
        const f32x4 w = ((const f32x4*)f.norm_w)[c];
        u32x2 pk;
        pk[0] = pack_bf2(v[0] * (1.0f + w[0]), v[1] * (1.0f + w[1]));
        pk[1] = pack_bf2(v[2] * (1.0f + w[2]), v[3] * (1.0f + w[3]));
        *(u32x2*)(xs + m * ldx + c * 4) = pk;
      }
      float ssum = 0.f;
      for (int i = t; i < f.ss_n; i += 256) ssum += f.ss_in[(size_t)m * f.ss_ld + i];
      ssum = wave_sum(ssum);
      if ((t & 63) == 0) red[(t >> 6) * 16 + m] = ssum;
    }
    __syncthreads();
    if (t < M) red[64 + t] = rsqrtf((red[t] + red[16 + t] + red[32 + t] + red[48 + t]) / (float)K + f.eps);
  } else if constexpr (PRO == 2) {
    // one pass per (row, head, 4 dims): merge over the splits, no LDS staging / barriers
    const int D = f.head_dim, G = f.q_per_kv, S = f.asplit;
    const int h0 = k0 / D, nh = Kr / D, D4 = D >> 2;
    const int items = M * nh * D4;
    if (S <= 16) {
      // every split's (m, l, o) loaded at once (one dependent L2 round trip, no read of the kv length:
      // splits past it hold m = -inf and weigh 0), then a two-pass max / weighted sum
      for (int idx = t; idx < M * nh * D4; idx += 256) {
        const int m = idx / (nh * D4), rem = idx % (nh * D4), hl = rem / D4, d4 = rem % D4;
        const int hq = h0 + hl;
        const long base0 = (((long)m * f.kv_heads + hq / G) * S) * 16 + (hq % G);
        float ms[16], ls[16];
        f32x4 o4[16];
        f32x2 mlv[16];
        // all 32 loads issued back to back before any is used (sched_barrier): the scheduler otherwise recycled
        // one register for six of the O loads, a load -> wait -> load chain of six round trips
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) {
          const long bs = base0 + (long)min(sp, S - 1) * 16;
          mlv[sp] = *(const f32x2*)(f.part_ml + bs * 2);
          o4[sp] = *(const f32x4*)(f.part_o + bs * f.dtw + d4 * 4);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) {
          ms[sp] = sp < S ? mlv[sp][0] : -INFINITY;
          ls[sp] = mlv[sp][1];
        }
        float mx = ms[0];
#pragma unroll
        for (int sp = 1; sp < 16; ++sp) mx = fmaxf(mx, ms[sp]);
        float den = 0.f;
        f32x4 num = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sp = 0; sp < 16; ++sp) {
          const float w = ms[sp] == -INFINITY ? 0.f : exp2f(ms[sp] - mx);
          den += w * ls[sp];
          num += w * o4[sp];
        }
        const float inv = 1.0f / den;
        u32x2 pk;
        pk[0] = pack_bf2(num[0] * inv, num[1] * inv);
        pk[1] = pack_bf2(num[2] * inv, num[3] * inv);
        *(u32x2*)(xs + m * ldx + hl * D + d4 * 4) = pk;
      }
      __syncthreads();
      return;
    }
    const int Seff = (f.slot_dev && f.akeys > 0) ? min(S, (*f.slot_dev + f.akeys) / f.akeys) : S;
    // one (row, head, 4 dims) item merged over its first Sn splits
    auto merge_item = [&](int idx, int m, int Sn) {
      const int rem = idx % (nh * D4), hl = rem / D4, d4 = rem % D4;
      const int hq = h0 + hl;
      const long base0 = (((long)m * f.kv_heads + hq / G) * S) * 16 + (hq % G);
      float mx = -INFINITY, den = 0.f;
      f32x4 num = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int sp = 0; sp < Sn; ++sp) {
        const long bs = base0 + (long)sp * 16;
        const float ms = f.part_ml[bs * 2], ls = f.part_ml[bs * 2 + 1];
        const f32x4 o4 = *(const f32x4*)(f.part_o + bs * f.dtw + d4 * 4);
        const float mn = fmaxf(mx, ms);
        const float ca = mx == -INFINITY ? 0.f : exp2f(mx - mn);
        const float cb = ms == -INFINITY ? 0.f : exp2f(ms - mn);
        den = den * ca + cb * ls;
        num = num * ca + cb * o4;
        mx = mn;
      }
      const float inv = 1.0f / den;
      u32x2 pk;
      pk[0] = pack_bf2(num[0] * inv, num[1] * inv);
      pk[1] = pack_bf2(num[2] * inv, num[3] * inv);
      *(u32x2*)(xs + m * ldx + hl * D + d4 * 4) = pk;
    };
    if (e.slot_rows) {
      // PG_SLOT_ROWS: row m's own count, its kv length before this token being slot_dev[m] + slot_base (a branch on
      // a kernel argument: the shared-length loop below keeps its wave-uniform trip count)
      for (int idx = t; idx < items; idx += 256) {
        const int m = idx / (nh * D4);
        merge_item(idx, m, min(S, (f.slot_dev[m] + f.slot_base + f.akeys) / f.akeys));
      }
    } else {
      for (int idx = t; idx < items; idx += 256) merge_item(idx, idx / (nh * D4), Seff);
    }
  }
  __syncthreads();
}

// The tail both block decodes share: pair P = 4(2h + s) + p of a block becomes dword p of operand op[h][s].  e holds the
// pair's two exponent codes in the exponent field's place of a bf16 pair; base (badd = base << 7 in both halves) is
// added to each, or with Z -- the block holds a code 0, exponent field 0 -- only to the codes that are not 0.
template <bool Z>
__device__ __forceinline__ void w_pair(const u32x4 (&sm)[2], int P, unsigned e, unsigned base, unsigned badd,
                                       u32x4 (&op)[2][2]) {
  if constexpr (Z) {
    const unsigned nz = ((e + 0x0f800f80u) >> 5) & 0x00800080u;   // 1 << 7 per half whose code is not 0
    e += __umul24(nz, base);
  } else {
    e += badd;
  }
  const int h = P >> 3, s = (P >> 2) & 1, p = P & 3;
  // sm dword p = bytes (s 0, o 0), (s 1, o 0), (s 0, o 1), (s 1, o 1): each byte doubled into its half-word puts the
  // sign at bit 15 and the mantissa at bits 0..6 (one v_perm), the rest is masked off as the exponent goes in
  const unsigned x = sm[h][p];
  const unsigned d = __builtin_amdgcn_perm(x, x, s == 0 ? 0x02020000u : 0x03030101u);
  op[h][s][p] = (d & 0x807f807fu) | e;
}

// PG_W_FRAG13 (FRAG == 2; include/pghip.h): one lane's share of a 16-row x 128-k block, 13 dwords for 32 weights -- the
// sign/mantissa bytes of the block's two 64-k chunks, the 5-bit exponent codes, and the block's base | zflag << 8 word
struct W13 {
  u32x4 sm[2];
  u32x4 cq;
  unsigned c4;
  unsigned bz;
};
// The block's four MFMA operands op[h][s], bit for bit the u32x4 pieces the PG_W_FRAG layout holds for chunk h, piece
// s.  Z: the block holds a code 0 (exponent field 0: no base added to that weight); wave-uniform, from the base table.
template <bool Z>
__device__ __forceinline__ void decode13(const W13& b, unsigned bm, u32x4 (&op)[2][2]) {
  unsigned q[5] = {b.cq[0], b.cq[1], b.cq[2], b.cq[3], b.c4};
  // (opaque copies: the compiler otherwise hoists the 20 shifts both decodes share above their branch and keeps them
  // live across it -- 12 to 20 more VGPRs per kernel, one wave per SIMD fewer on q|k|v and the finalised down)
#pragma unroll
  for (int d = 0; d < 5; ++d) asm volatile("" : "+v"(q[d]));
  const unsigned badd = bm * 0x00800080u;              // (base - 1) << 7 in both halves (scalar)
#pragma unroll
  for (int P = 0; P < 16; ++P) {
    // the pair's two codes at bits 7..11 and 23..27, the exponent field's place in a bf16 pair
    unsigned e;
    if (P < 15) {
      const unsigned w = q[P / 3];
      e = (P % 3 == 0 ? w << 7 : P % 3 == 1 ? w << 2 : w >> 3) & 0x0f800f80u;
    } else {
      e = ((q[0] >> 8) & 0x00800080u) | ((q[1] >> 7) & 0x01000100u) | ((q[2] >> 6) & 0x02000200u) |
          ((q[3] >> 5) & 0x04000400u) | ((q[4] >> 4) & 0x08000800u);
    }
    w_pair<Z>(b.sm, P, e, bm, badd, op);
  }
}

// PG_W_FRAG12 (FRAG == 3; include/pghip.h): the same block in 12 dwords per lane -- the sign/mantissa bytes and four
// dwords of 4-bit codes -- plus, for a wide block only, the dword of its 5-bit codes' top bits from the heap (a narrow
// block's c5 is the heap's shared line 0, loaded and never read)
struct W12 {
  u32x4 sm[2];
  u32x4 cq;
  unsigned c5;
};
// The block's four MFMA operands, as decode13.  MODE 0: narrow, exponent field = code + bias; 1: wide, 5-bit codes, no
// code 0, field = code + bias; 2: wide with a code 0 (field 0, bias left out).  Wave-uniform, from the block's table word.
template <int MODE>
__device__ __forceinline__ void decode12(const W12& b, unsigned bias, u32x4 (&op)[2][2]) {
  unsigned q[4] = {b.cq[0], b.cq[1], b.cq[2], b.cq[3]};
  unsigned c5 = 0;
  // (opaque copies, as in decode13: the shifts the three decodes share stay inside their branches)
#pragma unroll
  for (int d = 0; d < 4; ++d) asm volatile("" : "+v"(q[d]));
  if constexpr (MODE > 0) {
    c5 = b.c5;
    asm volatile("" : "+v"(c5));
  }
  const unsigned badd = bias * 0x00800080u;             // bias << 7 in both halves (scalar)
#pragma unroll
  for (int P = 0; P < 16; ++P) {
    // pair P = 4(2h + s) + p: its two 4-bit codes, nibble p of either half of q[2h + s], go to bits 7..10 and 23..26
    const unsigned w = q[P >> 2];
    unsigned e = ((P & 3) == 0 ? w << 7 : (P & 3) == 1 ? w << 3 : (P & 3) == 2 ? w >> 1 : w >> 5) & 0x07800780u;
    if constexpr (MODE > 0)                             // ... and a wide block's fifth bits, c5 bits P and 16 + P, to 11 and 27
      e |= (P < 11 ? c5 << (11 - P) : c5 >> (P - 11)) & 0x08000800u;
    w_pair<MODE == 2>(b.sm, P, e, bias, badd, op);
  }
}
