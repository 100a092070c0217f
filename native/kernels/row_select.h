// Row-pass helpers shared by the sampler (sampling.hip) and the logprob kernel
// (logit_ops.hip): one 1024-thread workgroup per [cols] bf16 row, an
// order-preserving 16-bit key per logit, and 256-bin LDS count histograms (high
// byte, then low byte) that find the k-th largest key exactly without a sort.
//
// The templates take the kernel's own __shared__ struct S; it must have
//   unsigned cnt[256 * NCOPY], bc[256];  float sv[16];  int si[16], sel[4];
#pragma once

#include "kgs_common.h"

namespace kgs {
namespace smp {

constexpr int NT = 1024;    // threads per row
constexpr int NCOPY = 16;   // histogram copies
constexpr int NONE = 0x7fffffff;
constexpr unsigned KEY_FINITE = 0x0080;  // the smallest key above -inf's (0x007f)

// bf16 bits -> 16-bit key, larger value = larger key (-0 counts as +0)
__device__ __forceinline__ unsigned key16(unsigned short h) {
  if (h == 0x8000) h = 0;
  return (h & 0x8000) ? (unsigned)(~h & 0xffff) : (unsigned)(h | 0x8000);
}
__device__ __forceinline__ unsigned short unkey16(unsigned k) {
  return (unsigned short)((k & 0x8000) ? (k & 0x7fff) : (~k & 0xffff));
}

// argmax_rows' order: NaN beats everything, then the value, then the lower index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// f(chunk index, the chunk's 8 logits) over this thread's 16-B chunks of a row.
// Eight loads in flight with clamped indices, as argmax_rows issues them.
template <bool STREAM, class F>
__device__ __forceinline__ void for_chunks(const bf16x8* xr, int nch, int t, F&& f) {
  for (int c0 = t; c0 < nch; c0 += NT * 8) {
    bf16x8 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16x8* p = xr + min(c0 + NT * j, nch - 1);
      v[j] = STREAM ? __builtin_nontemporal_load(p) : *p;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + NT * j;
      if (c >= nch) break;
      f(c, v[j]);
    }
  }
}

// the block's best (value, index) in every thread
template <class S>
__device__ __forceinline__ void block_best(float& bv, int& bi, S& sh, int t) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if ((t & 63) == 0) sh.sv[t >> 6] = bv, sh.si[t >> 6] = bi;
  __syncthreads();
  bv = sh.sv[0], bi = sh.si[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w)
    if (better(sh.sv[w], sh.si[w], bv, bi)) bv = sh.sv[w], bi = sh.si[w];
  __syncthreads();
}

template <class S>
__device__ __forceinline__ void zero_counts(S& sh, int t) {
#pragma unroll
  for (int j = 0; j < 256 * NCOPY / NT; ++j) sh.cnt[t + NT * j] = 0;
}

// The bin holding the k-th largest element of the count histogram (1 <= k <=
// the histogram's total), and how many of the k lie inside that bin.
template <class S>
__device__ __forceinline__ int select_count(S& sh, unsigned k, unsigned& inside, int t) {
  __syncthreads();
  if (t < 256) {
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < NCOPY; ++j) s += sh.cnt[t * NCOPY + j];
    sh.bc[t] = s;
  }
  __syncthreads();
  if (t < 256) {
    unsigned above = 0;
    for (int j = t + 1; j < 256; ++j) above += sh.bc[j];
    if (above < k && above + sh.bc[t] >= k) sh.sel[0] = t, sh.sel[1] = (int)(k - above);
  }
  __syncthreads();
  inside = (unsigned)sh.sel[1];
  return sh.sel[0];
}

}  // namespace smp
}  // namespace kgs
