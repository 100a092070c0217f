// What the optimizer's kernel files share (optimizer.hip: the bf16-gradient step,
// grad_accum.hip: fp32 main gradients): the tensor table's row, the state block,
// the table search, the global-memory accessors and the update of one element.
// The layouts are documented at the top of optimizer.hip.
#pragma once
#include "kgs_common.h"

#define KGS_ADAMW_CHUNK 16384

namespace kgs {
namespace opt {

constexpr int CHUNK = KGS_ADAMW_CHUNK;
constexpr int THREADS = 256;
constexpr int SPAN = THREADS * 8;  // elements one trip of the workgroup covers

struct Row {
  unsigned short* w;
  float* p;
  float* m;
  float* v;
  const unsigned short* g;  // the fp32 main gradient in a main table (grad_accum.hip casts it)
  long numel;
  long group;
  long chunk0;
};
static_assert(sizeof(Row) == 64, "table row layout");

struct State {
  int step;
  int skipped;
  float grad_norm;
  float clip;
  float bc1;
  float bc2;
  int skip;
  int micro;  // grad_accum.hip: micro-batches pending (> 0) or consumed by the last step (<= 0)
};
static_assert(sizeof(State) == 32, "state block layout");

// the last row whose chunk0 <= chunk: rows without chunks (numel 0) share their
// chunk0 with the next row and are passed over
__device__ __forceinline__ int find_row(const Row* __restrict__ rows, int n, long chunk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].chunk0 <= chunk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The tensors' pointers come out of the table, so hipcc cannot know their address
// space and would emit flat_ loads and stores; they are global memory.
template <bool NT, class T>
__device__ __forceinline__ T ld(const T* p) {
  const KGS_GLB T* q = (const KGS_GLB T*)p;
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

template <bool NT, class T>
__device__ __forceinline__ void st(T* p, T v) {
  KGS_GLB T* q = (KGS_GLB T*)p;
  if constexpr (NT) __builtin_nontemporal_store(v, q);
  else *q = v;
}

// ---------------------------------------------------------------------------
// The update of one element. The constants are wave-uniform and made once per
// thread in double: k1 = (1 - b1) clip and k2 = (1 - b2) clip^2 as unevaluated
// fp32 pairs (hi + lo), decay = 1 - lr wd rounded once. With main gradients
// clip stands for clip * s, s the micro-batch average's 1 / n.
//
// m' = b1 m + k1 g cancels when the gradient turns against the momentum, and a
// rounded product k1 g would then leave an error that is relative to the
// product, not to m'. So the product's own rounding error (one fma) and the
// low half of k1 are added back after the sum: m' and v' carry two roundings of
// the RESULT, |err| <= 2^-23 |m'|, for any clip. g^2 is exact in fp32 for a
// bf16 gradient (8 significant bits). An fp32 main gradient has 24, and g * g
// then rounds once: an error of 2^-24 g^2 k2 <= 2^-24 |v'| (every term of v' is
// non-negative, so k2 g^2 <= v'), which the tests' 2^-22 |v'| still covers.
struct Consts {
  float b1, b2, k1h, k1l, k2h, k2l, decay, lr, bc1, bc2, eps;
};

__device__ __forceinline__ void update(const Consts& c, float g, float& p, float& m, float& v) {
  const float t1 = c.k1h * g;
  const float e1 = __builtin_fmaf(c.k1l, g, __builtin_fmaf(c.k1h, g, -t1));
  m = __builtin_fmaf(c.b1, m, t1) + e1;
  const float g2 = g * g;
  const float t2 = c.k2h * g2;
  const float e2 = __builtin_fmaf(c.k2l, g2, __builtin_fmaf(c.k2h, g2, -t2));
  v = __builtin_fmaf(c.b2, v, t2) + e2;
  const float u = (m / c.bc1) / (__builtin_sqrtf(v / c.bc2) + c.eps);
  p = __builtin_fmaf(p, c.decay, -(c.lr * u));
}

}  // namespace opt
}  // namespace kgs
