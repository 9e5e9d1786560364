// Constrained decoding on the device (gfx950): a DFA over token classes restricts what a decode step may pick.
//
//   pg_dfa_mask     : before the sampler -- every token the row's DFA state does not allow gets a -inf logit.
//   pg_dfa_advance  : after the sampler  -- the row's state follows the token that was picked.
//
// The grammar is two int16 tables (pghip/grammar.py TokenDFA): cls [V], the class of every token id (class 0 = never
// allowed), and trans [S][C], the next state or -1.  Token t is allowed in state s iff trans[s][cls[t]] >= 0; there is
// no per-state bitmask over the vocabulary.  A row's state is one int32 word on the device; a negative state (and one
// >= S) means "free": the row is not constrained and stays so.  Both launches read the state words from the device
// and have a fixed grid, so a decode step with them is graph-capturable.
//
// Plain C++ throughout; every store is a vector store (the error word included).
#include "common.h"

#define DM_CHUNKS 64            // workgroups per row, as argmax_partial_kernel
#define DM_MAX_C 4096           // classes: the allowed bitmap is DM_MAX_C / 8 = 512 bytes of LDS
#define DM_MAX_S 32767
#define DM_MAX_B 1024

struct DmArgs {
  float* x;
  long ld;
  int V;
  const int16_t* cls;
  const int16_t* trans;
  int S, C;
  const int* state;
};

// bit c of `live`: class c is allowed (a class outside [0, C) never is: validate() rules it out, this keeps a bad table
// from reading past the bitmap)
__device__ __forceinline__ bool dm_dead(const uint32_t* live, int C, int16_t c) {
  const uint32_t u = (uint32_t)(int)c;
  return u >= (uint32_t)C || !((live[u >> 5] >> (u & 31)) & 1u);
}

// One workgroup per (chunk, row).  The row's trans row becomes a C-bit bitmap in LDS (a wave's ballot over 64 classes
// is two words of it); the chunk's classes then stream in as 16-byte loads of 8, and the kernel only stores: -inf over
// four consecutive dead tokens as one 16-byte store where the address is 16-byte aligned, single stores otherwise.
// The logits are never read, so every other word keeps its bits.  Chunks are multiples of 8 tokens, so with a 16-byte
// aligned cls (CVEC) every full group of 8 loads aligned; the ragged end of a row is scalar.
template <bool CVEC>
__global__ __launch_bounds__(256) void dfa_mask_kernel(DmArgs a) {
  __shared__ uint32_t live[DM_MAX_C / 32];
  const int b = blockIdx.y, ch = blockIdx.x;
  const int s = a.state[b];
  if (s < 0 || s >= a.S) return;                   // a free row: not touched at all
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C;
  const int16_t* tr = a.trans + (long)s * C;
  for (int base = wave * 64; base < C; base += 256) {
    const int c = base + lane;
    const unsigned long long m = __ballot(c < C && tr[c] >= 0);
    if (lane == 0) {
      live[base >> 5] = (uint32_t)m;
      live[(base >> 5) + 1] = (uint32_t)(m >> 32);
    }
  }
  __syncthreads();
  const int V = a.V;
  const int per = ((V + DM_CHUNKS - 1) / DM_CHUNKS + 7) & ~7;
  const long s0 = (long)ch * per;
  const long e = min((long)V, s0 + per);
  float* row = a.x + (long)b * a.ld;
  const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (long i = s0 + tid * 8; i < e; i += 256 * 8) {
    if (i + 7 < e) {
      int16_t c[8];
      if (CVEC) {
        const u32x4 q = *(const u32x4*)(a.cls + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c[2 * j] = (int16_t)(q[j] & 0xffffu);
          c[2 * j + 1] = (int16_t)(q[j] >> 16);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = a.cls[i + j];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bool d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = dm_dead(live, C, c[4 * h + j]);
        float* p = row + i + 4 * h;
        if (d[0] && d[1] && d[2] && d[3] && ((uintptr_t)p & 15) == 0) {
          *(f32x4*)p = ninf;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (d[j]) p[j] = -INFINITY;
        }
      }
    } else {
      for (long t = i; t < e; ++t)
        if (dm_dead(live, C, a.cls[t])) row[t] = -INFINITY;
    }
  }
}

static inline bool dm_tables_ok(const void* cls, const void* trans, int B, int V, int S, int C) {
  return cls && trans && B >= 1 && B <= DM_MAX_B && V >= 1 && S >= 1 && S <= DM_MAX_S && C >= 2 && C <= DM_MAX_C &&
         ((uintptr_t)cls & 1) == 0 && ((uintptr_t)trans & 1) == 0;
}

extern "C" int pg_dfa_mask(float* logits, long ld, int B, int V, const int16_t* cls, const int16_t* trans, int S, int C,
                           const int* state, hipStream_t stream) {
  PG_REQUIRE(logits && state && dm_tables_ok(cls, trans, B, V, S, C));
  PG_REQUIRE((B == 1 || ld >= V) && ((uintptr_t)logits & 3) == 0 && ((uintptr_t)state & 3) == 0);
  const DmArgs a{logits, ld, V, cls, trans, S, C, state};
  if (((uintptr_t)cls & 15) == 0)
    hipLaunchKernelGGL(dfa_mask_kernel<true>, dim3(DM_CHUNKS, B), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(dfa_mask_kernel<false>, dim3(DM_CHUNKS, B), dim3(256), 0, stream, a);
  PG_LAUNCH_CHECK();
  return 0;
}

// One workgroup, one thread per row.  A free row stays free; a token the state does not allow, a class or a next state
// outside the tables, and an id outside [0, V) leave the state where it is and set *err (every thread that sets it
// stores the same 1, so the order of those stores does not matter).
__global__ __launch_bounds__(DM_MAX_B) void dfa_advance_kernel(int* __restrict__ state, const int64_t* __restrict__ ids,
                                                               int B, int V, const int16_t* __restrict__ cls,
                                                               const int16_t* __restrict__ trans, int S, int C,
                                                               int* __restrict__ err) {
  const int b = threadIdx.x;
  if (b >= B) return;
  const int s = state[b];
  if (s < 0 || s >= S) return;
  const int64_t t = ids[b];
  int n = -1;
  if (t >= 0 && t < V) {
    const int c = cls[t];
    if (c >= 0 && c < C) n = trans[(long)s * C + c];
  }
  if (n >= 0 && n < S)
    state[b] = n;
  else
    *err = 1;
}

extern "C" int pg_dfa_advance(int* state, const int64_t* ids, int B, int V, const int16_t* cls, const int16_t* trans,
                              int S, int C, int* err, hipStream_t stream) {
  PG_REQUIRE(state && ids && err && dm_tables_ok(cls, trans, B, V, S, C));
  PG_REQUIRE(((uintptr_t)state & 3) == 0 && ((uintptr_t)ids & 7) == 0 && ((uintptr_t)err & 3) == 0);
  hipLaunchKernelGGL(dfa_advance_kernel, dim3(1), dim3((B + 63) & ~63), 0, stream, state, ids, B, V, cls, trans, S, C,
                     err);
  PG_LAUNCH_CHECK();
  return 0;
}
