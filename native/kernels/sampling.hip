// Fused token sampler for gfx950: temperature, top-k, top-p and a counter-based
// random draw for every row of a [rows, cols] bf16 logits matrix in ONE launch,
// greedy rows included (they get argmax_rows' answer).
//
// One 1024-thread workgroup per row. A 128k-vocabulary row is 256 KB: it does
// not fit in LDS, so the kernel makes up to five passes over a row that stays
// in L2 / MALL after the first. Nothing is sorted:
//
//   pass 1  argmax (first index of the maximum, NaN counts as the maximum) and,
//           with top-k on, a 256-bin count histogram of the keys' high bytes
//   pass 2  top-k: count histogram of the low bytes inside the bin that holds
//           the k-th largest key -> the exact k-th largest logit
//   pass 3  top-p: fixed-point mass histogram of the survivors' high bytes
//   pass 4  top-p: counts of the low bytes inside the bin where the cumulative
//           mass crosses p; a bin is one bf16 value, so its mass is
//           count * weight(value) -> the exact smallest kept logit
//   pass 5  Gumbel-max over the kept set with Philox4x32-10 uniforms; a cheap
//           upper bound of each candidate's score skips the accurate logarithms
//           for the candidates that cannot win
//
// bf16 has 65 536 values, so an order-preserving 16-bit key and two 256-bin
// levels (high byte, low byte) select exactly. Masses are integers (weights
// scaled by 2^40, u64 LDS adds), so the accumulation order does not matter and
// identical inputs give identical outputs. Histograms are kept in 16 copies
// (one per lane & 15): logits crowd into a handful of exponent bins, and the
// copies keep a wave's adds to one bin on different LDS banks.
//
// Semantics (kgs.ops.transformer.sample_rows_reference states them in numpy):
//   * temperature <= 0, a NaN in the row, or no finite maximum: argmax_rows' answer
//   * top-k on when 0 < k < cols: keep logits >= the k-th largest (ties kept)
//   * top-p on when 0 < p < 1, after top-k: with M(v) the softmax(x / T) mass of
//     the survivors strictly greater than v, keep a token iff M(its logit) < p
//   * token = argmax_i (x_i / T + g_i), lowest index first, g_i = -log(-log(u_i)),
//     u_i = ((w >> 8) + 0.5) * 2^-24, w = word i % 4 of Philox4x32-10 with key
//     (seed lo, seed hi) and counter (i / 4, counter lo, counter hi, 0)
#include "row_select.h"  // keys, for_chunks, block_best, the count-histogram select

namespace kgs {
namespace smp {

// softmax weight of logit x against the row maximum m, as an integer: exp((x - m) / T) * 2^40
__device__ __forceinline__ unsigned long long weight(float x, float m, float T) {
  return (unsigned long long)(__expf((x - m) / T) * 1099511627776.f);
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned* w) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// -log(-log(u)), u = ((w >> 8) + 0.5) * 2^-24. n + 0.5 has 25 significant bits
// for n >= 2^23: there the inner log goes through 1 - u, which is exact in fp32.
__device__ __forceinline__ float gumbel(unsigned w) {
  const unsigned n = w >> 8;
  float e;
  if (n < (1u << 23))
    e = -logf(__builtin_fmaf((float)n, 0x1p-24f, 0x1p-25f));
  else
    e = -log1pf(-(((float)((1u << 24) - n) - 0.5f) * 0x1p-24f));
  return -logf(e);
}

// float bits -> unsigned of the same order, and back
__device__ __forceinline__ unsigned ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
}

struct Shared {
  unsigned cnt[256 * NCOPY];
  unsigned long long mass[256 * NCOPY];
  unsigned long long bm[256];
  unsigned bc[256];
  float sv[16];
  int si[16];
  int sel[4];
  unsigned bound;  // pass 5: the best perturbed score any thread has reached so far (ordered())
  unsigned long long sel_above, sel_total;
};

__global__ __launch_bounds__(1024) void sample_rows(const unsigned short* __restrict__ x, long long* __restrict__ out,
                                                    const float* __restrict__ temperature,
                                                    const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                    const long long* __restrict__ seed,
                                                    const long long* __restrict__ counter, int cols, long ld) {
  __shared__ Shared sh;
  const int row = blockIdx.x, t = threadIdx.x, cp = t & (NCOPY - 1);
  const bf16x8* xr = (const bf16x8*)(x + row * ld);
  const int nch = cols / 8;
  const float T = temperature[row], p = top_p[row];
  const int k = top_k[row];
  const bool sampled = T > 0.f;
  const bool kf = sampled && k > 0 && k < cols;
  const bool pf = sampled && p > 0.f && p < 1.f;

  // pass 1: argmax (+ the top-k level-1 histogram)
  if (kf) zero_counts(sh, t);
  __syncthreads();
  float bv = -INFINITY;
  int bi = NONE;
  for_chunks<false>(xr, nch, t, [&](int c, bf16x8 v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned short h = (unsigned short)v[e];
      const float f = bf2f(h);
      if (better(f, 8 * c + e, bv, bi)) bv = f, bi = 8 * c + e;
      if (kf) atomicAdd(&sh.cnt[(key16(h) >> 8) * NCOPY + cp], 1u);
    }
  });
  block_best(bv, bi, sh, t);
  const int amax = bi == NONE ? 0 : bi;
  const float m = bv;
  if (!sampled || m != m || fabsf(m) == INFINITY) {  // greedy, a NaN in the row, no finite maximum
    if (t == 0) out[row] = amax;
    return;
  }

  // top-k: the key of the k-th largest logit (never below the smallest finite key: -inf is never kept)
  unsigned kk = KEY_FINITE;
  if (kf) {
    unsigned inside, unused;
    const unsigned hb = (unsigned)select_count(sh, (unsigned)k, inside, t);
    zero_counts(sh, t);
    __syncthreads();
    for_chunks<false>(xr, nch, t, [&](int, bf16x8 v) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned key = key16((unsigned short)v[e]);
        if ((key >> 8) == hb) atomicAdd(&sh.cnt[(key & 255) * NCOPY + cp], 1u);
      }
    });
    const unsigned lb = (unsigned)select_count(sh, inside, unused, t);
    kk = max(kk, (hb << 8) | lb);
  }

  // top-p: the smallest key whose mass-above is below p
  unsigned kf_key = kk;
  if (pf) {
#pragma unroll
    for (int j = 0; j < 256 * NCOPY / NT; ++j) sh.mass[t + NT * j] = 0;
    __syncthreads();
    for_chunks<false>(xr, nch, t, [&](int, bf16x8 v) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned short h = (unsigned short)v[e];
        const unsigned key = key16(h);
        if (key >= kk) atomicAdd(&sh.mass[(key >> 8) * NCOPY + cp], weight(bf2f(h), m, T));
      }
    });
    __syncthreads();
    if (t < 256) {
      unsigned long long s = 0;
#pragma unroll
      for (int j = 0; j < NCOPY; ++j) s += sh.mass[t * NCOPY + j];
      sh.bm[t] = s;
    }
    __syncthreads();
    if (t < 256) {
      unsigned long long above = 0, total = 0;
      for (int j = 0; j < 256; ++j) {
        const unsigned long long b = sh.bm[j];
        total += b;
        if (j > t) above += b;
      }
      const double pz = (double)p * (double)total;
      // the first bin from the top where the cumulative mass reaches p: the boundary value lies in it
      if ((double)above < pz && (double)(above + sh.bm[t]) >= pz)
        sh.sel[0] = t, sh.sel_above = above, sh.sel_total = total;
    }
    __syncthreads();
    const unsigned hb = (unsigned)sh.sel[0];
    const unsigned long long above0 = sh.sel_above;
    const double pz = (double)p * (double)sh.sel_total;
    zero_counts(sh, t);
    __syncthreads();
    for_chunks<false>(xr, nch, t, [&](int, bf16x8 v) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned key = key16((unsigned short)v[e]);
        if (key >= kk && (key >> 8) == hb) atomicAdd(&sh.cnt[(key & 255) * NCOPY + cp], 1u);
      }
    });
    __syncthreads();
    if (t < 256) {
      unsigned s = 0;
#pragma unroll
      for (int j = 0; j < NCOPY; ++j) s += sh.cnt[t * NCOPY + j];
      // one bin = one bf16 value: its mass is count * weight(value)
      sh.bm[t] = s ? s * weight(bf2f(unkey16((hb << 8) | (unsigned)t)), m, T) : 0ull;
      if (t == 0) sh.sel[2] = 255;
    }
    __syncthreads();
    if (t < 256) {
      unsigned long long above = above0;
      for (int j = t + 1; j < 256; ++j) above += sh.bm[j];
      if ((double)above < pz) atomicMin(&sh.sel[2], t);
    }
    __syncthreads();
    kf_key = max(kk, (hb << 8) | (unsigned)sh.sel[2]);
  }

  // Gumbel-max over the kept set
  const unsigned long long sd = (unsigned long long)seed[row], ct = (unsigned long long)counter[row];
  const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32), c1 = (unsigned)ct, c2 = (unsigned)(ct >> 32);
  // The accurate logarithms are most of this pass's work and almost every
  // logit loses, so each candidate first gets an upper bound of its score from
  // the hardware logarithm (within 1e-4 of the accurate Gumbel term wherever
  // -log(u) > 1e-3; nearer to u = 1 no bound is taken) and is dropped when even
  // that, plus a margin of 0.01, stays below a score some thread has already
  // reached (sh.bound). A dropped candidate can neither win nor tie, so the
  // token is the one the full evaluation picks, whatever order the threads run in.
  if (t == 0) sh.bound = ordered(-INFINITY);
  __syncthreads();
  bv = -INFINITY;
  bi = NONE;
  for_chunks<true>(xr, nch, t, [&](int c, bf16x8 v) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) any |= key16((unsigned short)v[4 * half + e]) >= kf_key;
      if (!any) continue;
      unsigned w[4];
      philox4x32_10((unsigned)(2 * c + half), c1, c2, 0u, k0, k1, w);
      const float reached = unordered(sh.bound);
      const float before = bv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned short h = (unsigned short)v[4 * half + e];
        if (key16(h) < kf_key) continue;
        const float xs = bf2f(h) / T;
        const float ea = -__logf(__builtin_fmaf((float)(w[e] >> 8), 0x1p-24f, 0x1p-25f));
        if (ea > 1e-3f && xs - __logf(ea) + 0.01f < fmaxf(reached, bv)) continue;
        const float s = xs + gumbel(w[e]);
        const int i = 8 * c + 4 * half + e;
        if (better(s, i, bv, bi)) bv = s, bi = i;
      }
      if (bv > before && bv > reached) atomicMax(&sh.bound, ordered(bv));
    }
  });
  block_best(bv, bi, sh, t);
  if (t == 0) out[row] = bi == NONE ? amax : bi;
}

}  // namespace smp
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// logits: [rows, ld] bf16 (cols % 8 == 0, ld % 8 == 0, 16-B aligned); out: int64 [rows];
// temperature / top_p: fp32 [rows]; top_k: int32 [rows]; seed / counter: int64 [rows]
KGS_EXPORT int kgs_sample_rows_bf16(const void* logits, long long* out, const float* temperature, const int* top_k,
                                    const float* top_p, const long long* seed, const long long* counter, int rows,
                                    int cols, long ld, hipStream_t s) {
  if (rows < 0 || cols <= 0 || ld < cols) return KGS_ERR_SHAPE;
  if (cols % 8 || ld % 8 || !al16(logits)) return KGS_ERR_ALIGN;
  if (rows == 0) return 0;
  if (!logits || !out || !temperature || !top_k || !top_p || !seed || !counter) return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::smp::sample_rows, dim3(rows), dim3(kgs::smp::NT), 0, s, (const unsigned short*)logits, out,
                     temperature, top_k, top_p, seed, counter, cols, ld);
  return (int)hipGetLastError();
}
