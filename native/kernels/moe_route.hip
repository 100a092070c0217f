// Mixture-of-experts routing for gfx950: top-k selection with softmax weights,
// token-priority slot assignment on fixed-capacity slabs, the dispatch gather,
// the weighted combine, and their backwards. The FFNs themselves run as the
// existing GEMMs on row slices [e C, (e + 1) C) of the dispatched matrix.
//
//   * moe_select    : per row of logits [T, E] the k largest (ties to the lower
//                     index), fp32 softmax over the k winners.
//   * moe_hist / moe_scan / moe_slots : with f = t k + j the flat index,
//                     rank(f) = #{f' < f with the same e}; slot = e C + rank (or
//                     -1 past the capacity), src its inverse, counts per e.
//   * moe_gather    : xe[s] = x[src[s] / k] (bit copy, zero row for an empty
//                     slot); with a scale, bf16(scale[src[s]] x[src[s] / k]): dye.
//   * moe_combine   : y[t] = bf16(sum_j w[t, j] ye[slot[t, j]]), fp32 in ascending j,
//                     dropped j skipped; without weights it is dx of the gather.
//   * moe_dw        : dweights[t, j] = sum_c dy[t, c] ye[slot[t, j], c] in fp32.
//   * moe_route_bwd : dlogits[t, e_j] = w_j (dw_j - sum_i w_i dw_i), 0 elsewhere.
//
// House rules (attention_train.hip): fp32 math, one bf16 rounding per output
// element, 16-B accesses, no float atomics, no workgroup waits on another, every
// element of every output written on every call (no memset, nothing depends on
// what a buffer held before), nothing synchronises with the host.
//
// Select. G lanes own one row, one 16-B chunk of 8 logits each: G is E / 8 rounded
// up to a power of two (the spare lanes of a group hold empty keys), so a wave
// covers 64 / G rows per trip. A logit becomes a 32-bit key: the high half is the
// bf16 pattern made monotonic (sign fixed; -0 folded onto +0 so that the two tie;
// any NaN the largest, as torch.sort has it), the low half 0xFFFF - index. One
// unsigned max therefore picks the winner AND breaks ties towards the lower
// index, keys of a row are all different, and an empty key is 0. k rounds of an
// in-lane max over 8 keys and a DPP butterfly over the group (quad_perm x 2,
// row_half_mirror, row_mirror), the winner masked out after each: no LDS and no
// barrier. Every lane of the group ends with all k winners; lane 0 runs the
// softmax in registers and stores. A NaN row gets NaN weights and indices that
// are still decoded from keys, hence in range.
//
// Ranks. A workgroup owns RANK_BLK consecutive flat indices, a wave RANK_CPW
// consecutive chunks of 64 of them. Per chunk, for every distinct e present (the
// leading lane's, found with a ballot) the ballot of "mine == e" gives the in-wave
// rank through mbcnt and the chunk's total through a popcount; the total goes to
// the wave's own running [E] row in LDS. moe_hist adds the four waves' rows into
// the workgroup's histogram in the workspace; moe_scan (one workgroup) turns the
// histograms into exclusive bases over the workgroups and writes counts;
// moe_slots recomputes the wave rows, makes them running bases (workgroup base +
// earlier waves), walks the chunks again and writes slot and src, then fills the
// tail of every slab in src with -1. Integer arithmetic only, no atomics.
//
// Gather. Slot-major: a wave takes GROWS slots, src[s] is a scalar, a lane moves
// the 16-B chunks lane, lane + 64, ... of all GROWS rows, every load of a trip
// issued before its first store. Combine. Token-major: a wave owns 512 columns of
// one token (8 per lane); the k slots and weights are scalars and all k gathers
// are issued before the first fma. dweights. A wave per token, a lane's fp32
// sums over its chunks, then a wave sum in a fixed order (DPP within a row of 16,
// permlane swaps across). Indices read from memory (src, slot, experts) are
// range-checked before they address anything: a bad one counts as empty.
#include "kgs_common.h"

namespace kgs {
namespace moe {

constexpr int MAX_E = 128;
constexpr int MAX_K = 8;
constexpr int RANK_CPW = 4;                   // chunks of 64 flat indices per wave
constexpr int RANK_BLK = 4 * RANK_CPW * 64;   // flat indices per workgroup of the rank passes
constexpr int GROWS = 4;                      // slots per wave trip of the gather
constexpr int MAX_WGS = 8192;                 // grid cap of the grid-stride kernels

template <int CTRL>
__device__ __forceinline__ unsigned dppu(unsigned v) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// The max over the g lanes of a group (g a power of two up to 16), in all of them.
__device__ __forceinline__ unsigned group_max(unsigned v, int g) {
  if (g > 1) v = max(v, dppu<0xB1>(v));   // lane ^ 1
  if (g > 2) v = max(v, dppu<0x4E>(v));   // lane ^ 2
  if (g > 4) v = max(v, dppu<0x141>(v));  // row_half_mirror: the other quad of the eight
  if (g > 8) v = max(v, dppu<0x140>(v));  // row_mirror: the other eight of the row
  return v;
}

// The sum over the wave in a fixed order, in every lane.
__device__ __forceinline__ float wave_sum(float v) {
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x141>(v);
  v += dppf<0x140>(v);
  return xor32_sum(xor16_sum(v));
}

__device__ __forceinline__ unsigned make_key(unsigned short bits, int index) {
  unsigned b = bits;
  if ((b & 0x7fffu) == 0) b = 0;  // -0 ties with +0
  const unsigned h = (b & 0x7fffu) > 0x7f80u ? 0xffffu : (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
  return (h << 16) | (0xffffu - (unsigned)index);
}

__device__ __forceinline__ float key_value(unsigned key) {
  const unsigned h = key >> 16;  // 0xffff (a NaN) decodes to 0x7fff, a NaN
  return bf2f((unsigned short)((h & 0x8000u) ? (h & 0x7fffu) : (~h & 0xffffu)));
}

__global__ __launch_bounds__(256) void moe_select(const unsigned short* __restrict__ logits,
                                                  float* __restrict__ weights, int* __restrict__ experts, long T,
                                                  int E, int k, long ld, int g, int gshift) {
  const int L = E >> 3;
  const int lane = threadIdx.x & 63;
  const int c = lane & (g - 1);
  const int rpw = 64 >> gshift;  // rows per wave trip
  const long nwaves = (long)gridDim.x * 4;
  // the trip count is wave-uniform: every lane stays on for the DPP steps
  for (long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw; r0 < T; r0 += nwaves * rpw) {
    const long t = r0 + (lane >> gshift);
    unsigned key[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) key[e] = 0;
    if (t < T && c < L) {
      const bf16x8 v = *(const bf16x8*)(logits + t * ld + 8 * c);
#pragma unroll
      for (int e = 0; e < 8; ++e) key[e] = make_key((unsigned short)v[e], 8 * c + e);
    }
    unsigned win[MAX_K];
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      win[j] = 0;
      if (j < k) {
        unsigned m = key[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) m = max(m, key[e]);
        m = group_max(m, g);
        win[j] = m;
#pragma unroll
        for (int e = 0; e < 8; ++e) key[e] = key[e] == m ? 0u : key[e];
      }
    }
    if (t < T && c == 0) {
      const float v0 = key_value(win[0]);
      float p[MAX_K], sum = 0.f;
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        p[j] = j < k ? expf(key_value(win[j]) - v0) : 0.f;
        sum += p[j];
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        if (j < k) {
          weights[t * k + j] = p[j] * inv;
          experts[t * k + j] = (int)(0xffffu - (win[j] & 0xffffu));
        }
      }
    }
  }
}

// One wave's walk over its RANK_CPW chunks from flat index f0. run: the wave's own
// [E] row in LDS; on entry the rank of the wave's first occurrence of each e, on
// exit that plus the wave's totals. WRITE: slot and src are stored.
template <bool WRITE>
__device__ __forceinline__ void rank_walk(const int* __restrict__ experts, long n, long f0, int E, int C,
                                          volatile int* run, int* __restrict__ slot, int* __restrict__ src) {
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int ch = 0; ch < RANK_CPW; ++ch) {
    const long f = f0 + ch * 64 + lane;
    int e = -1;
    if (f < n) {
      e = experts[f];
      if ((unsigned)e >= (unsigned)E) e = -1;
    }
    unsigned long long rem = __ballot(e >= 0);
    int rank = 0;
    while (rem) {  // wave-uniform: one trip per distinct e of the chunk
      const int lead = __ffsll((unsigned long long)rem) - 1;
      const int el = __builtin_amdgcn_readlane(e, lead);
      const unsigned long long m = __ballot(e == el);
      const int base = run[el];
      if (e == el)
        rank = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      __builtin_amdgcn_wave_barrier();
      if (lane == lead) run[el] = base + (int)__popcll(m);
      __builtin_amdgcn_wave_barrier();
      rem &= ~m;
    }
    if (WRITE && f < n) {
      int sl = -1;
      if (e >= 0 && rank < C) {
        sl = e * C + rank;
        src[sl] = (int)f;
      }
      slot[f] = sl;
    }
  }
}

__global__ __launch_bounds__(256) void moe_hist(const int* __restrict__ experts, long n, int E, int* __restrict__ ws) {
  __shared__ int wh[4][MAX_E];
  for (int i = threadIdx.x; i < 4 * MAX_E; i += 256) (&wh[0][0])[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  rank_walk<false>(experts, n, (long)blockIdx.x * RANK_BLK + wave * (RANK_CPW * 64), E, 0, wh[wave], nullptr, nullptr);
  __syncthreads();
  if ((int)threadIdx.x < E)
    ws[(long)blockIdx.x * E + threadIdx.x] =
        wh[0][threadIdx.x] + wh[1][threadIdx.x] + wh[2][threadIdx.x] + wh[3][threadIdx.x];
}

// One workgroup: ws[g][e] (workgroup g's count of e) becomes the exclusive sum
// over g' < g, and counts[e] the total. Thread (s, e) owns segment s of the
// workgroups; the 1024 / E segment sums meet in LDS.
__global__ __launch_bounds__(1024) void moe_scan(int* __restrict__ ws, int* __restrict__ counts, int nwg, int E) {
  __shared__ int seg[1024];
  const int S = 1024 / E;
  const int e = threadIdx.x % E, s = threadIdx.x / E;
  const int per = (nwg + S - 1) / S;
  const int g0 = min(s * per, nwg), g1 = min(g0 + per, nwg);
  int sum = 0;
  if (s < S) {
    for (int g = g0; g < g1; ++g) sum += ws[g * E + e];
    seg[s * E + e] = sum;
  }
  __syncthreads();
  if (s < S) {
    int base = 0;
    for (int q = 0; q < s; ++q) base += seg[q * E + e];
    if (s == S - 1) counts[e] = base + sum;
    for (int g = g0; g < g1; ++g) {
      const int h = ws[g * E + e];
      ws[g * E + e] = base;
      base += h;
    }
  }
}

__global__ __launch_bounds__(256) void moe_slots(const int* __restrict__ experts, long n, int E, int C,
                                                 const int* __restrict__ ws, const int* __restrict__ counts,
                                                 int* __restrict__ slot, int* __restrict__ src) {
  __shared__ int wh[4][MAX_E];
  for (int i = threadIdx.x; i < 4 * MAX_E; i += 256) (&wh[0][0])[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const long f0 = (long)blockIdx.x * RANK_BLK + wave * (RANK_CPW * 64);
  rank_walk<false>(experts, n, f0, E, 0, wh[wave], nullptr, nullptr);
  __syncthreads();
  if ((int)threadIdx.x < E) {  // the waves' totals -> each wave's running base
    int b = ws[(long)blockIdx.x * E + threadIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int h = wh[w][threadIdx.x];
      wh[w][threadIdx.x] = b;
      b += h;
    }
  }
  __syncthreads();
  rank_walk<true>(experts, n, f0, E, C, wh[wave], slot, src);
  // the unfilled tail of every slab: min(count, C) .. C - 1
  const long total = (long)E * C;
  for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < total; s += (long)gridDim.x * 256) {
    const int e = (int)(s / C);
    if ((int)(s - (long)e * C) >= counts[e]) src[s] = -1;
  }
}

__global__ __launch_bounds__(256) void moe_gather(const unsigned short* __restrict__ x, const int* __restrict__ src,
                                                  const float* __restrict__ scale, unsigned short* __restrict__ out,
                                                  long nflat, long S, int k, int chunks, long ldx, long ldo) {
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  for (long s0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * GROWS; s0 < S; s0 += nwaves * GROWS) {
    long row[GROWS];
    float w[GROWS];
#pragma unroll
    for (int r = 0; r < GROWS; ++r) {
      int f = -1;
      if (s0 + r < S) f = __builtin_amdgcn_readfirstlane(src[s0 + r]);
      if ((unsigned long)(long)f >= (unsigned long)nflat) f = -1;
      row[r] = f < 0 ? -1 : (long)(f / k);
      w[r] = scale != nullptr && f >= 0 ? scale[f] : 1.f;
    }
    for (int c = lane; c < chunks; c += 64) {
      bf16x8 v[GROWS];
#pragma unroll
      for (int r = 0; r < GROWS; ++r) {
        v[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (row[r] >= 0) v[r] = *(const bf16x8*)(x + row[r] * ldx + 8 * c);
      }
      if (scale != nullptr) {
#pragma unroll
        for (int r = 0; r < GROWS; ++r) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = w[r] * bf2f((unsigned short)v[r][e]);
          if (row[r] >= 0) v[r] = pack_bf16x8(o, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < GROWS; ++r)
        if (s0 + r < S) *(bf16x8*)(out + (s0 + r) * ldo + 8 * c) = v[r];
    }
  }
}

// The k slots (and weights) of token t, as scalars (SCALAR) or one copy per lane
// (moe_dw: its eight row addresses as scalars would spill SGPRs); a dropped or bad
// slot is -1.
template <bool SCALAR>
__device__ __forceinline__ void token_slots(int (&sl)[MAX_K], float (&w)[MAX_K], const int* __restrict__ slot,
                                            const float* __restrict__ weights, long t, int k, long S) {
#pragma unroll
  for (int j = 0; j < MAX_K; ++j) {
    sl[j] = -1;
    w[j] = 1.f;
    if (j < k) {
      const int s = SCALAR ? __builtin_amdgcn_readfirstlane(slot[t * k + j]) : slot[t * k + j];
      if ((unsigned long)(long)s < (unsigned long)S) {
        sl[j] = s;
        if (weights != nullptr) {
          const int wb = __builtin_bit_cast(int, weights[t * k + j]);
          w[j] = __builtin_bit_cast(float, SCALAR ? __builtin_amdgcn_readfirstlane(wb) : wb);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void moe_combine(const unsigned short* __restrict__ ye,
                                                   const int* __restrict__ slot, const float* __restrict__ weights,
                                                   unsigned short* __restrict__ y, long T, long S, int k, int D,
                                                   int nslice, long ldye, long ldy) {
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4, items = T * nslice;
  for (long it = (long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {
    const long t = it / nslice;
    const int col = (int)(it - t * nslice) * 512 + 8 * lane;
    int sl[MAX_K];
    float w[MAX_K];
    token_slots<true>(sl, w, slot, weights, t, k, S);
    if (col < D) {
      bf16x8 v[MAX_K];
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        v[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (sl[j] >= 0) v[j] = *(const bf16x8*)(ye + (long)sl[j] * ldye + col);
      }
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        if (sl[j] >= 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(w[j], bf2f((unsigned short)v[j][e]), acc[e]);
        }
      }
      *(bf16x8*)(y + t * ldy + col) = pack_bf16x8(acc, 0);
    }
  }
}

__global__ __launch_bounds__(256) void moe_dw(const unsigned short* __restrict__ dy,
                                              const unsigned short* __restrict__ ye, const int* __restrict__ slot,
                                              float* __restrict__ dweights, long T, long S, int k, int chunks,
                                              long lddy, long ldye) {
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += nwaves) {
    int sl[MAX_K];
    float w[MAX_K], acc[MAX_K];
    token_slots<false>(sl, w, slot, nullptr, t, k, S);
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) acc[j] = 0.f;
    for (int c = lane; c < chunks; c += 64) {
      const bf16x8 g = *(const bf16x8*)(dy + t * lddy + 8 * c);
      bf16x8 v[MAX_K];
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        v[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (sl[j] >= 0) v[j] = *(const bf16x8*)(ye + (long)sl[j] * ldye + 8 * c);
      }
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        if (sl[j] >= 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc[j] = __builtin_fmaf(bf2f((unsigned short)g[e]), bf2f((unsigned short)v[j][e]), acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      if (j < k) {  // wave-uniform
        const float s = wave_sum(acc[j]);
        if (lane == 0) dweights[t * k + j] = sl[j] >= 0 ? s : 0.f;
      }
    }
  }
}

// A thread owns one 16-B chunk of one row of dlogits.
__global__ __launch_bounds__(256) void moe_route_bwd(const float* __restrict__ dweights,
                                                     const float* __restrict__ weights,
                                                     const int* __restrict__ experts,
                                                     unsigned short* __restrict__ dlogits, long T, int E, int k,
                                                     long ld) {
  const int L = E >> 3;
  const long total = T * L;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long t = i / L;
    const int c = (int)(i - t * L);
    float w[MAX_K], d[MAX_K], dot = 0.f;
    int rel[MAX_K];
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      w[j] = d[j] = 0.f;
      rel[j] = -1;
      if (j < k) {
        w[j] = weights[t * k + j];
        d[j] = dweights[t * k + j];
        rel[j] = experts[t * k + j] - 8 * c;
        dot = __builtin_fmaf(w[j], d[j], dot);
      }
    }
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      const float val = w[j] * (d[j] - dot);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rel[j] == e ? val : o[e];
    }
    *(bf16x8*)(dlogits + t * ld + 8 * c) = pack_bf16x8(o, 0);
  }
}

static inline int capped(long want) { return (int)(want < 1 ? 1 : (want < MAX_WGS ? want : MAX_WGS)); }

}  // namespace moe
}  // namespace kgs

static inline bool moe_al(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p & (a - 1)) == 0; }

// T tokens, E choices (a multiple of 8 in 8 .. 128), k picks per token (1 .. min(8, E)).
static inline int moe_route_shape(long T, int E, int k) {
  if (T < 1 || E < 8 || E > kgs::moe::MAX_E || E % 8 || k < 1 || k > kgs::moe::MAX_K || k > E) return KGS_ERR_SHAPE;
  if (T > 0x7fffffffL / k) return KGS_ERR_SHAPE;  // flat indices are 32-bit
  return 0;
}

// T tokens, S = E C slots, k picks, D columns (a multiple of 8).
static inline int moe_rows_shape(long T, long S, int k, int D) {
  if (T < 1 || S < 1 || S > 0x7fffffffL || k < 1 || k > kgs::moe::MAX_K || D < 8 || D % 8) return KGS_ERR_SHAPE;
  if (T > 0x7fffffffL / k) return KGS_ERR_SHAPE;
  return 0;
}

// Bytes of the int32 workspace kgs_moe_route_bf16 needs (one [E] histogram per
// workgroup of the rank passes), or KGS_ERR_SHAPE. At least 16.
KGS_EXPORT long kgs_moe_workspace(long T, int E, int k) {
  if (moe_route_shape(T, E, k)) return KGS_ERR_SHAPE;
  const long nwg = (T * k + kgs::moe::RANK_BLK - 1) / kgs::moe::RANK_BLK;
  const long b = nwg * E * 4;
  return b < 16 ? 16 : b;
}

// logits: bf16 [T, ld]. weights: fp32 [T, k]; experts, slot: int32 [T, k]; src:
// int32 [E C]; counts: int32 [E]; all contiguous and all written in full. ws:
// kgs_moe_workspace(T, E, k) bytes. Four launches.
KGS_EXPORT int kgs_moe_route_bf16(const void* logits, float* weights, int* experts, int* slot, int* src, int* counts,
                                  void* ws, long T, int E, int k, int C, long ld, hipStream_t s) {
  using namespace kgs::moe;
  if (const int rc = moe_route_shape(T, E, k)) return rc;
  if (C < 1 || (long)E * C > 0x7fffffffL || ld < E) return KGS_ERR_SHAPE;
  if (!moe_al(logits, 16) || !moe_al(weights, 4) || !moe_al(experts, 4) || !moe_al(slot, 4) || !moe_al(src, 4) ||
      !moe_al(counts, 4) || !moe_al(ws, 4) || ld % 8)
    return KGS_ERR_ALIGN;
  int g = 1, gshift = 0;
  while (g < E / 8) g <<= 1, ++gshift;
  const long n = T * k;
  const int rpw = 64 / g, nwg = (int)((n + RANK_BLK - 1) / RANK_BLK);
  hipLaunchKernelGGL(moe_select, dim3(capped((T + 4 * rpw - 1) / (4 * rpw))), dim3(256), 0, s,
                     (const unsigned short*)logits, weights, experts, T, E, k, ld, g, gshift);
  hipLaunchKernelGGL(moe_hist, dim3(nwg), dim3(256), 0, s, (const int*)experts, n, E, (int*)ws);
  hipLaunchKernelGGL(moe_scan, dim3(1), dim3(1024), 0, s, (int*)ws, counts, nwg, E);
  hipLaunchKernelGGL(moe_slots, dim3(nwg), dim3(256), 0, s, (const int*)experts, n, E, C, (const int*)ws,
                     (const int*)counts, slot, src);
  return (int)hipGetLastError();
}

// dlogits: bf16 [T, ld], every one of its E columns written (0 where the row did
// not pick the column). dweights, weights: fp32 [T, k]; experts: int32 [T, k].
KGS_EXPORT int kgs_moe_route_bwd_bf16(const float* dweights, const float* weights, const int* experts, void* dlogits,
                                      long T, int E, int k, long ld, hipStream_t s) {
  using namespace kgs::moe;
  if (const int rc = moe_route_shape(T, E, k)) return rc;
  if (ld < E) return KGS_ERR_SHAPE;
  if (!moe_al(dweights, 4) || !moe_al(weights, 4) || !moe_al(experts, 4) || !moe_al(dlogits, 16) || ld % 8)
    return KGS_ERR_ALIGN;
  hipLaunchKernelGGL(moe_route_bwd, dim3(capped((T * (E / 8) + 255) / 256)), dim3(256), 0, s, dweights, weights,
                     experts, (unsigned short*)dlogits, T, E, k, ld);
  return (int)hipGetLastError();
}

// out[s] = x[src[s] / k] for s < S, a zero row where src[s] < 0; with scale (fp32
// by flat index) bf16(scale[src[s]] x[src[s] / k]). x: bf16 [T, ldx]; out: bf16
// [S, ldo]; D columns. out must not overlap x.
KGS_EXPORT int kgs_moe_gather_bf16(const void* x, const int* src, const float* scale, void* out, long T, long S,
                                   int k, int D, long ldx, long ldo, hipStream_t s) {
  using namespace kgs::moe;
  if (const int rc = moe_rows_shape(T, S, k, D)) return rc;
  if (ldx < D || ldo < D) return KGS_ERR_SHAPE;
  if (!moe_al(x, 16) || !moe_al(src, 4) || !moe_al(out, 16) || ((uintptr_t)scale & 3) || ldx % 8 || ldo % 8)
    return KGS_ERR_ALIGN;
  hipLaunchKernelGGL(moe_gather, dim3(capped((S + 4 * GROWS - 1) / (4 * GROWS))), dim3(256), 0, s,
                     (const unsigned short*)x, src, scale, (unsigned short*)out, T * k, S, k, D / 8, ldx, ldo);
  return (int)hipGetLastError();
}

// y[t] = bf16(sum_j weights[t, j] ye[slot[t, j]]) over the j with slot >= 0;
// weights may be null (all 1: the gather's dx). ye: bf16 [S, ldye]; y: bf16 [T, ldy].
KGS_EXPORT int kgs_moe_combine_bf16(const void* ye, const int* slot, const float* weights, void* y, long T, long S,
                                    int k, int D, long ldye, long ldy, hipStream_t s) {
  using namespace kgs::moe;
  if (const int rc = moe_rows_shape(T, S, k, D)) return rc;
  if (ldye < D || ldy < D) return KGS_ERR_SHAPE;
  if (!moe_al(ye, 16) || !moe_al(slot, 4) || !moe_al(y, 16) || ((uintptr_t)weights & 3) || ldye % 8 || ldy % 8)
    return KGS_ERR_ALIGN;
  const int nslice = (D + 511) / 512;
  hipLaunchKernelGGL(moe_combine, dim3(capped((T * nslice + 3) / 4)), dim3(256), 0, s, (const unsigned short*)ye, slot,
                     weights, (unsigned short*)y, T, S, k, D, nslice, ldye, ldy);
  return (int)hipGetLastError();
}

// The combine's backward: dye [S, lddye] = bf16(weights[src[s]] dy[src[s] / k])
// (exact zeros at empty slots) and dweights [T, k] fp32 = dy[t] . ye[slot[t, j]]
// (0 for a dropped j). Two launches.
KGS_EXPORT int kgs_moe_combine_bwd_bf16(const void* dy, const void* ye, const int* slot, const int* src,
                                        const float* weights, void* dye, float* dweights, long T, long S, int k,
                                        int D, long lddy, long ldye, long lddye, hipStream_t s) {
  using namespace kgs::moe;
  if (const int rc = moe_rows_shape(T, S, k, D)) return rc;
  if (lddy < D || ldye < D || lddye < D) return KGS_ERR_SHAPE;
  if (!moe_al(dy, 16) || !moe_al(ye, 16) || !moe_al(slot, 4) || !moe_al(src, 4) || !moe_al(weights, 4) ||
      !moe_al(dye, 16) || !moe_al(dweights, 4) || lddy % 8 || ldye % 8 || lddye % 8)
    return KGS_ERR_ALIGN;
  hipLaunchKernelGGL(moe_gather, dim3(capped((S + 4 * GROWS - 1) / (4 * GROWS))), dim3(256), 0, s,
                     (const unsigned short*)dy, src, weights, (unsigned short*)dye, T * k, S, k, D / 8, lddy, lddye);
  hipLaunchKernelGGL(moe_dw, dim3(capped((T + 3) / 4)), dim3(256), 0, s, (const unsigned short*)dy,
                     (const unsigned short*)ye, slot, dweights, T, S, k, D / 8, lddy, ldye);
  return (int)hipGetLastError();
}
