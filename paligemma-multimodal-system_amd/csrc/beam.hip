// Beam search on the device (gfx950): candidate selection and the KV-cache reorder that follows it.
//
//   pg_beam_select     : from W rows of logits per prompt, the best W of the W*V candidates cum[parent] +
//                        log_softmax(logits[parent])[token]; finished beams frozen; advances the decode state as
//                        pg_argmax does.  Two launches, logits read once.
//   pg_kv_beam_gather  : row r's generated keys / values become what row parent[r] held, in k, vt, kd and vd, for all
//                        layers.  Two launches through a suffix-sized scratch, so any parent map is legal.
//
// Plain C++ throughout; every store is a vector store.  Nothing here orders candidates by a float atomic: the only
// atomic is an integer count of finished rows in LDS, whose result does not depend on the order of its additions.
#include "common.h"

// ---------------------------------------------------------------- selection
// A candidate travels as one 64-bit word, larger = better: the logit's order-preserving key in the high half and
// ~token in the low half, so that of two equal logits the lower token is the larger word ("first index on ties", as
// pg_argmax).  Keys: 0 = no candidate, 1 = a NaN logit (below every comparable value, -inf included, but still a real
// token: a row of nothing but NaN yields W valid ids), else the usual sign-flipped float bits with -0 folded onto +0.
#define BS_CHUNKS 64           // workgroups per row (= lanes of the wave that merges a row)
#define BS_MAXW 8
#define BS_NV 4                // 16-byte vectors a thread holds per tile
#define BS_TILE (256 * 4 * BS_NV)
typedef unsigned long long bs_u64;

__device__ __forceinline__ uint32_t bs_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  const uint32_t k = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  return v == v ? k : 1u;
}
__device__ __forceinline__ float bs_unkey(uint32_t k) {
  if (k <= 1u) return NAN;
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bs_u64 bs_wave_max(bs_u64 c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const bs_u64 x = __shfl_xor(c, o, 64);
    c = x > c ? x : c;
  }
  return c;
}
// (m, s) <- online-softmax merge; an empty side has m = -inf, s = 0 (pg_token_logprob's rule)
__device__ __forceinline__ void bs_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - M)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - M));
  m = M;
}

struct BsPartArgs {
  const float* x;
  long ld;
  int V, W;
  const int* finished;
  float* pm;       // [rows][BS_CHUNKS] chunk max
  float* ps;       // [rows][BS_CHUNKS] chunk sum of exp(x - max); NaN when the chunk holds a NaN
  bs_u64* pc;      // [rows][BS_CHUNKS][W] the chunk's best W candidates, best first
};

// One workgroup per (chunk, row).  Per tile of 4096 columns a thread holds its 16 logits as keys in registers; each
// wave then takes its best W in W rounds of (local best, wave maximum, strike the winner), with the best W of the
// earlier tiles riding along in lanes 0..W-1 (`carry`), so a chunk of any length needs W words per wave.
template <bool VEC>
__global__ __launch_bounds__(256) void beam_partial_kernel(BsPartArgs a) {
  __shared__ float sm[4], ss[4];
  __shared__ bs_u64 sc[4 * BS_MAXW];
  const int r = blockIdx.y, ch = blockIdx.x, W = a.W;
  if (a.finished[r]) return;                       // a frozen beam offers (row, pad) only: its logits are not read
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = ((a.V + BS_CHUNKS - 1) / BS_CHUNKS + 3) & ~3;
  const long s0 = (long)ch * per;
  const int e = (int)min((long)a.V, s0 + per);
  const float* row = a.x + (long)r * a.ld;
  float m = -INFINITY, s = 0.f;
  bool bad = false;
  bs_u64 carry = 0;
  for (long t0 = s0; t0 < e; t0 += BS_TILE) {
    uint32_t key[4 * BS_NV];
#pragma unroll
    for (int v = 0; v < BS_NV; ++v) {
      const long i = t0 + (long)(v * 256 + tid) * 4;
      float x[4];
      if (VEC && i + 3 < e) {
        const f32x4 q = *(const f32x4*)(row + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = q[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = i + j < e ? row[i + j] : -INFINITY;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t k = i + j < e ? bs_key(x[j]) : 0u;
        key[v * 4 + j] = k;
        bad |= k == 1u;
      }
      const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
      if (mx > m) {
        s *= __expf(m - mx);
        m = mx;
      }
      if (m != -INFINITY) s += (__expf(x[0] - m) + __expf(x[1] - m)) + (__expf(x[2] - m) + __expf(x[3] - m));
    }
    bs_u64 next = 0;
    for (int rd = 0; rd < W; ++rd) {
      uint32_t bk = 0;
      int bj = 0;
#pragma unroll
      for (int j = 4 * BS_NV - 1; j >= 0; --j)
        if (key[j] >= bk) { bk = key[j]; bj = j; }          // (>= walking down: the lowest column among equals)
      const uint32_t col = (uint32_t)(t0 + (long)((bj >> 2) * 256 + tid) * 4 + (bj & 3));
      bs_u64 c = bk ? ((bs_u64)bk << 32) | (0xffffffffu - col) : 0;
      c = carry > c ? carry : c;
      c = bs_wave_max(c);
      if (lane == rd) next = c;
      if (carry == c) carry = 0;
      const uint32_t wcol = 0xffffffffu - (uint32_t)c;
#pragma unroll
      for (int j = 0; j < 4 * BS_NV; ++j) {
        const uint32_t cj = (uint32_t)(t0 + (long)((j >> 2) * 256 + tid) * 4 + (j & 3));
        if (c != 0 && cj == wcol) key[j] = 0;
      }
    }
    carry = next;
  }
  if (bad) { s = NAN; m = m == -INFINITY ? 0.f : m; }   // a NaN logit makes the row's log-sum-exp NaN whatever it sits among
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bs_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane == 0) { sm[wave] = m; ss[wave] = s; }
  if (lane < W) sc[wave * BS_MAXW + lane] = carry;
  __syncthreads();
  if (wave != 0) return;
  bs_u64 c = lane < 4 * W ? sc[(lane / W) * BS_MAXW + lane % W] : 0;
  bs_u64 mine = 0;
  for (int rd = 0; rd < W; ++rd) {
    const bs_u64 w = bs_wave_max(c);
    if (lane == rd) mine = w;
    if (c == w) c = 0;
  }
  if (lane < W) a.pc[((long)r * BS_CHUNKS + ch) * W + lane] = mine;
  if (lane == 0) {
    for (int w = 1; w < 4; ++w) bs_merge(m, s, sm[w], ss[w]);
    a.pm[r * BS_CHUNKS + ch] = m;
    a.ps[r * BS_CHUNKS + ch] = s;
  }
}

struct BsFinalArgs {
  const float* pm;
  const float* ps;
  const bs_u64* pc;
  float* rm;        // [rows] row max
  float* rl;        // [rows] log of the row's sum of exp(x - max)
  bs_u64* rc;       // [rows][W] the row's best W candidates, best first
  int B, W, V;
  float* cum;
  int* finished;
  int stop_token, pad_token;
  int64_t* out_ids;
  int* parent;
  int64_t* hist_tok;
  int* hist_parent;
  int hist_rows;
  int* step;
  int* pos;
  int* kv_len;
  int* flag;
};

// One workgroup.  Phase A, a wave per live row: merge the row's 64 chunk records (lane = chunk) into its log-sum-exp
// and best W candidates.  Phase B, a wave per prompt: lane i*W + j holds candidate j of parent i, ranks it among the
// group's W*W by counting the lanes that beat it, and the lanes ranked below W write the group's new rows.
// cum / finished in place: a wave reads its whole group's values before the rank count (whose shuffles need every
// lane's score) and writes after it, and no wave reads another group's rows.
__global__ __launch_bounds__(1024) void beam_final_kernel(BsFinalArgs a) {
  __shared__ int nfin;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int W = a.W, rows = a.B * W;
  const int st = a.step ? *a.step : 0;
  if (threadIdx.x == 0) nfin = 0;
  for (int p = wave; p < rows; p += nw) {
    if (a.finished[p]) continue;
    const float m = a.pm[p * BS_CHUNKS + lane];
    const float M = wave_max(m);
    const float S = wave_sum(m == -INFINITY ? 0.f : a.ps[p * BS_CHUNKS + lane] * __expf(m - M));
    bs_u64 c[BS_MAXW];
#pragma unroll
    for (int j = 0; j < BS_MAXW; ++j) c[j] = j < W ? a.pc[((long)p * BS_CHUNKS + lane) * W + j] : 0;
    bs_u64 mine = 0;
    for (int rd = 0; rd < W; ++rd) {
      bs_u64 b = c[0];
#pragma unroll
      for (int j = 1; j < BS_MAXW; ++j) b = c[j] > b ? c[j] : b;
      b = bs_wave_max(b);
      if (lane == rd) mine = b;
#pragma unroll
      for (int j = 0; j < BS_MAXW; ++j)
        if (c[j] == b) c[j] = 0;
    }
    if (lane < W) a.rc[(long)p * W + lane] = mine;
    if (lane == 0) { a.rm[p] = M; a.rl[p] = __logf(S); }
  }
  __syncthreads();                                  // phase A's records (global, same workgroup) and nfin = 0
  for (int g = wave; g < a.B; g += nw) {
    const int i = lane / W, j = lane % W;
    const bool in = lane < W * W;
    const int p = g * W + (in ? i : 0);
    const int fin = a.finished[p];
    const float c0 = a.cum[p];
    bool valid = in;
    float score = c0;
    int tok = a.pad_token;
    if (fin) {
      valid = valid && j == 0;
    } else {
      const bs_u64 c = a.rc[(long)p * W + j];
      const float x = bs_unkey((uint32_t)(c >> 32));
      const float M = a.rm[p];
      tok = (int)(0xffffffffu - (uint32_t)c);
      if (c == 0 || tok < 0 || tok >= a.V) tok = 0;               // (cannot happen with W <= V; never an id outside)
      // (x - M first, as pg_token_logprob: exact near the maximum); a row of nothing but -inf scores -inf
      score = M == -INFINITY ? -INFINITY : c0 + ((x - M) - a.rl[p]);
    }
    uint32_t sk = valid ? bs_key(score) : 0u;
    int rank = 0;
    for (int o = 0; o < 64; ++o) {
      const uint32_t ok = __shfl(sk, o, 64);
      rank += (ok > sk) || (ok == sk && o < lane);   // lane order is (parent, then the row's own order): lower (p, t) first
    }
    if (valid && rank < W) {
      const int o = g * W + rank;
      const int nf = fin || (a.stop_token >= 0 && tok == a.stop_token);
      a.out_ids[o] = tok;
      a.parent[o] = p;
      a.cum[o] = score;
      a.finished[o] = nf;
      if (st < a.hist_rows) {
        if (a.hist_tok) a.hist_tok[(long)st * rows + o] = tok;
        if (a.hist_parent) a.hist_parent[(long)st * rows + o] = p;
      }
      if (a.pos) a.pos[o] += 1;
      if (nf) atomicAdd(&nfin, 1);
    }
  }
  __syncthreads();                                  // every wave has read *step; nfin is complete
  if (threadIdx.x == 0) {
    if (a.kv_len) *a.kv_len += 1;
    if (a.step) *a.step = st + 1;
    if (a.flag) *a.flag = nfin == rows;
  }
}

static inline long bs_up16(long x) { return (x + 15) & ~15L; }

// workspace (16-B aligned), for rows = B * W: pm, ps [rows][64] floats; pc [rows][64][W] and rc [rows][W] 64-bit
// words; rm, rl [rows] floats (pghip/ops.py beam_select_workspace)
extern "C" int pg_beam_select(const float* logits, long ld, int V, int B, int W, float* cum, int* finished,
                              int stop_token, int pad_token, void* workspace, int64_t* out_ids, int* parent,
                              int64_t* hist_tok, int* hist_parent, int hist_rows, int* step, int* pos, int* kv_len,
                              int* flag, hipStream_t stream) {
  PG_REQUIRE(logits && cum && finished && workspace && out_ids && parent && V > 0 && B > 0);
  PG_REQUIRE(W >= 1 && W <= BS_MAXW && W <= V && (long)B * W <= 1024);
  const int rows = B * W;
  PG_REQUIRE((rows == 1 || ld >= V) && pad_token >= 0 && pad_token < V && stop_token < V);
  PG_REQUIRE(((hist_tok == nullptr && hist_parent == nullptr) || hist_rows > 0));
  PG_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out_ids & 7) == 0 &&
             ((uintptr_t)hist_tok & 7) == 0);
  char* w = (char*)workspace;
  float* pm = (float*)w;
  float* ps = pm + (long)rows * BS_CHUNKS;
  w += bs_up16((long)rows * BS_CHUNKS * 8);
  bs_u64* pc = (bs_u64*)w;
  w += (long)rows * BS_CHUNKS * W * 8;
  bs_u64* rc = (bs_u64*)w;
  w += (long)rows * W * 8;
  float* rm = (float*)w;
  float* rl = rm + rows;
  const BsPartArgs pa{logits, ld, V, W, finished, pm, ps, pc};
  // 16-B loads where every chunk of every row starts 16-B aligned (chunks are multiples of 4 columns)
  if (((uintptr_t)logits & 15) == 0 && ld % 4 == 0)
    hipLaunchKernelGGL(beam_partial_kernel<true>, dim3(BS_CHUNKS, rows), dim3(256), 0, stream, pa);
  else
    hipLaunchKernelGGL(beam_partial_kernel<false>, dim3(BS_CHUNKS, rows), dim3(256), 0, stream, pa);
  const BsFinalArgs fa{pm, ps, pc, rm, rl, rc, B, W, V, cum, finished, stop_token, pad_token, out_ids, parent,
                       hist_tok, hist_parent, hist_rows, step, pos, kv_len, flag};
  const int nw = rows < 1 ? 1 : (rows > 16 ? 16 : rows);
  hipLaunchKernelGGL(beam_final_kernel, dim3(1), dim3(64 * nw), 0, stream, fa);
  PG_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- KV reorder
// Row r's window of positions [lo, hi), lo = floor32(base[r]), hi = ceil32(len[r]) (clamped to Smax and to the scratch's
// S_scr positions), is copied from row parent[r] in 16-byte units.  Each layout holds n * kvd / 8 units per (layer,
// row), n = hi - lo:
//   k  [Smax][kvd]        : the window is one contiguous run;
//   vt [kvd][Smax]        : n / 8 units per dimension (lo is a multiple of 32, so every run starts 64-B aligned);
//   kd, vd [Hkv][Smax][D] : whole 32-key blocks of 32 * D elements (dec_koff / dec_voff), n * D / 8 units per kv head.
// The scratch has the same four layouts with Smax -> S_scr and positions counted from lo.  Launch 1 (to_scratch) reads
// row parent[r] of the cache into scratch row r; launch 2 reads scratch row r into cache row r: no launch reads what it
// writes, so swaps and cycles are as legal as the identity.  Rows with parent[r] == r and rows with no generated key
// (len <= base) are skipped by both.
struct KvgArgs {
  bf16_t* c[4];       // k, vt, kd, vd
  bf16_t* s[4];       // the scratch's four
  int layers, rows, Smax, Hkv, D, S_scr;
  const int* parent;
  const int* base;
  const int* len_dev;
  int len_rows, len_base;
  int to_scratch;
};

__device__ __forceinline__ long kvg_off(int q, long u, int n, int lo, int S, int kvd, int D) {
  if (q == 0) return ((long)lo * kvd) + u * 8;
  if (q == 1) {
    const long d = u / (n >> 3), w = u % (n >> 3);
    return d * S + lo + w * 8;
  }
  const long per = (long)n * (D >> 3);
  const long h = u / per, w = u % per;
  return h * S * D + (long)lo * D + w * 8;
}

__global__ __launch_bounds__(256) void kv_beam_gather_kernel(KvgArgs a) {
  const int r = blockIdx.y, layer = blockIdx.z;
  const int p = a.parent[r];
  if (p == r || p < 0 || p >= a.rows) return;
  const int base = a.base[r];
  const int len = a.len_base + (a.len_rows ? a.len_dev[r] : a.len_dev[0]);
  if (len <= base || base < 0) return;
  const int lo = base & ~31;
  int hi = (len + 31) & ~31;
  hi = min(hi, min(a.Smax, lo + a.S_scr));
  const int n = hi - lo;
  if (n <= 0) return;
  const int kvd = a.Hkv * a.D;
  const long units = (long)n * (kvd >> 3);
  const long rowsz = (long)a.Smax * kvd, srowsz = (long)a.S_scr * kvd;
  const long src_row = a.to_scratch ? p : r;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < 4 * units; t += (long)gridDim.x * 256) {
    const int q = (int)(t / units);
    const long u = t % units;
    const long co = kvg_off(q, u, n, lo, a.Smax, kvd, a.D);
    const long so = kvg_off(q, u, n, 0, a.S_scr, kvd, a.D);
    if (a.to_scratch) {
      const u32x4 v = *(const u32x4*)(a.c[q] + ((long)layer * a.rows + src_row) * rowsz + co);
      *(u32x4*)(a.s[q] + ((long)layer * a.rows + r) * srowsz + so) = v;
    } else {
      const u32x4 v = *(const u32x4*)(a.s[q] + ((long)layer * a.rows + r) * srowsz + so);
      *(u32x4*)(a.c[q] + ((long)layer * a.rows + r) * rowsz + co) = v;
    }
  }
}

// scratch: 4 * layers * rows * S_scr * Hkv * D bf16, 16-B aligned
extern "C" int pg_kv_beam_gather(void* k, void* vt, void* kd, void* vd, int layers, int rows, int Smax, int Hkv, int D,
                                 const int* parent, const int* base, const int* len_dev, int len_rows, int len_base,
                                 void* scratch, int S_scr, hipStream_t stream) {
  PG_REQUIRE(k && vt && kd && vd && parent && base && len_dev && scratch);
  PG_REQUIRE(layers > 0 && layers <= 65535 && rows > 0 && rows <= 65535 && Hkv > 0 && D > 0 && D % 8 == 0);
  PG_REQUIRE(Smax > 0 && Smax % 32 == 0 && S_scr >= 32 && S_scr % 32 == 0);
  PG_REQUIRE((((uintptr_t)k | (uintptr_t)vt | (uintptr_t)kd | (uintptr_t)vd | (uintptr_t)scratch) & 15) == 0);
  const long kvd = (long)Hkv * D;
  bf16_t* s0 = (bf16_t*)scratch;
  const long sz = (long)layers * rows * S_scr * kvd;
  KvgArgs a{{(bf16_t*)k, (bf16_t*)vt, (bf16_t*)kd, (bf16_t*)vd}, {s0, s0 + sz, s0 + 2 * sz, s0 + 3 * sz},
            layers, rows, Smax, Hkv, D, S_scr, parent, base, len_dev, len_rows, len_base, 1};
  const long units = 4L * min(S_scr, Smax) * (kvd / 8);              // the widest window a row can have
  long gx = (units + 256 * 4 - 1) / (256 * 4);                       // about four units per thread
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  hipLaunchKernelGGL(kv_beam_gather_kernel, dim3((unsigned)gx, rows, layers), dim3(256), 0, stream, a);
  a.to_scratch = 0;
  hipLaunchKernelGGL(kv_beam_gather_kernel, dim3((unsigned)gx, rows, layers), dim3(256), 0, stream, a);
  PG_LAUNCH_CHECK();
  return 0;
}
