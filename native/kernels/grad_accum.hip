// Gradient accumulation for gfx950: fp32 main gradients that the optimizer owns,
// summed over the micro-batches of a step, and the AdamW step that reads them.
//
//   * grad_accumulate : per element main = float(g_bf16) on the first micro-batch
//                       of a cycle, main = main + float(g_bf16) afterwards (one
//                       fp32 add), and zero bits into g_bf16 in the same pass
//   * micro_advance   : one thread, behind grad_accumulate on its stream: the
//                       micro-batch count of the state block goes up by one
//   * main_sumsq      : grad_sumsq (optimizer.hip) on the fp32 main gradients
//   * finalize_main   : finalize (optimizer.hip) with the norm scaled by s, and
//                       the cycle marked consumed
//   * adamw_step_main : adamw_step (optimizer.hip) with g = clip * s * main
//
// s = 1 / n for an averaged step, n the micro-batches accumulated, and 1 otherwise.
//
// Two tensor tables of optimizer.hip's layout with the same numel, group and
// chunk0 per row, so that row i and chunk c mean the same in both: the bf16
// table's word 4 is the gradient (0: none this micro-batch), the main table's
// word 4 the fp32 main gradient (in the step's table 0: no gradient in the
// whole cycle, the tensor is skipped).
//
// The micro-batch count is word 7 of the state block, `micro`:
//     micro > 0   that many micro-batches are summed in main and wait for a step
//     micro <= 0  the cycle is consumed: the next grad_accumulate overwrites main.
//                 finalize_main leaves -n, which adamw_step_main reads for s.
// Neither "first micro-batch" nor s is a kernel argument, so one captured
// accumulate and one captured step replay cycles of any length. Every workgroup
// of grad_accumulate reads micro; only micro_advance, ordered behind all of them
// by the stream, writes it. No atomics, no workgroup waits on another.
//
// Thread ownership and the order of every sum are those of optimizer.hip, and
// the update is the same update(): a cycle of one micro-batch (main = float(g),
// s = 1) is bit for bit the bf16 step. House rules as there.
#include "optimizer_common.h"

namespace kgs {
namespace opt {

// the __global__ functions of this file, template instantiations counted once
// each (tests/test_grad_accum.py compares it with what the compiler reports)
constexpr int KERNEL_COUNT = 6;

__device__ __forceinline__ float* main_of(const Row& r) {
  return reinterpret_cast<float*>(const_cast<unsigned short*>(r.g));
}

// ---------------------------------------------------------------------------
// U 16-B gradient groups per thread and trip (two 16-B main-gradient accesses
// each): all loads of a trip are issued before the first use. FIRST: main is
// not read. !HASG: zeros into main (the caller asks for that on a first
// micro-batch only). The chunk's short last group is done element by element by
// the thread that owns it.
template <bool FIRST, bool ZERO, bool HASG, int U>
__device__ __forceinline__ void accumulate_chunk(unsigned short* g, float* a, long i, long end) {
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (; i + (long)(U - 1) * SPAN + 8 <= end; i += (long)U * SPAN) {
    bf16x8 gv[U];
    f32x4 av[U][2];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long k = i + (long)j * SPAN;
      if constexpr (HASG) gv[j] = ld<false>((const bf16x8*)(g + k));
      else gv[j] = z8;
      if constexpr (!FIRST) {
        av[j][0] = ld<false>((const f32x4*)(a + k));
        av[j][1] = ld<false>((const f32x4*)(a + k) + 1);
      }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long k = i + (long)j * SPAN;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float f = bf2f((unsigned short)gv[j][4 * h + e]);
          if constexpr (FIRST) o[e] = f;
          else o[e] = av[j][h][e] + f;
        }
        st<false>((f32x4*)(a + k) + h, o);
      }
      if constexpr (ZERO && HASG) st<false>((bf16x8*)(g + k), z8);
    }
  }
  if constexpr (U > 1) {
    accumulate_chunk<FIRST, ZERO, HASG, 1>(g, a, i, end);
  } else {
    for (; i < end; ++i) {
      float f = 0.f;
      if constexpr (HASG) f = bf2f(ld<false>(g + i));
      if constexpr (FIRST) st<false>(a + i, f);
      else st<false>(a + i, ld<false>(a + i) + f);
      if constexpr (ZERO && HASG) st<false>(g + i, (unsigned short)0);
    }
  }
}

template <bool ZERO>
__global__ __launch_bounds__(THREADS) void grad_accumulate(const Row* __restrict__ grows,
                                                           const Row* __restrict__ mrows, int n,
                                                           const State* __restrict__ state) {
  const bool first = state->micro <= 0;
  const long chunk = blockIdx.x;
  const int t = find_row(mrows, n, chunk);
  const Row r = mrows[t];
  unsigned short* g = const_cast<unsigned short*>(grows[t].g);
  float* a = main_of(r);
  const long off = (chunk - r.chunk0) * CHUNK;
  if (off >= r.numel) return;
  const long end = r.numel - off < CHUNK ? r.numel : off + CHUNK;
  const long i = off + 8L * threadIdx.x;
  if (g == nullptr) {  // contributes nothing; a first micro-batch must not leave the old sum
    if (first) accumulate_chunk<true, false, false, 4>(nullptr, a, i, end);
    return;
  }
  if (first) accumulate_chunk<true, ZERO, true, 4>(g, a, i, end);
  else accumulate_chunk<false, ZERO, true, 4>(g, a, i, end);
}

__global__ __launch_bounds__(64) void micro_advance(State* __restrict__ state) {
  if (threadIdx.x != 0) return;
  const int m = state->micro;
  state->micro = m > 0 ? m + 1 : 1;
}

// ---------------------------------------------------------------------------
// grad_sumsq on fp32 values: a thread owns the same 8-element groups tid,
// tid + 256, ... of the chunk (two 16-B loads each, all issued before the first
// use) and adds their squares in the same order.
template <bool NT>
__global__ __launch_bounds__(THREADS) void main_sumsq(const Row* __restrict__ rows, int n,
                                                      float* __restrict__ partials) {
  __shared__ float red[THREADS / 64];
  const long chunk = blockIdx.x;
  const Row r = rows[find_row(rows, n, chunk)];
  const float* a = main_of(r);
  const long off = (chunk - r.chunk0) * CHUNK;
  float s = 0.f;
  if (a != nullptr && off < r.numel) {
    const long end = r.numel - off < CHUNK ? r.numel : off + CHUNK;
    const long i0 = off + 8L * threadIdx.x;
    constexpr int T = CHUNK / SPAN;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 av[T][2];
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const long i = i0 + (long)j * SPAN;
      const bool in = i + 8 <= end;
      av[j][0] = in ? ld<NT>((const f32x4*)(a + i)) : z4;
      av[j][1] = in ? ld<NT>((const f32x4*)(a + i) + 1) : z4;
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = av[j][e >> 2][e & 3];
        s += f * f;
      }
    }
    const long t0 = end & ~7L;  // the short group, if any, starts here
    if (t0 < end && (int)(((t0 - off) >> 3) % THREADS) == (int)threadIdx.x) {
      for (long i = t0; i < end; ++i) {
        const float f = ld<false>(a + i);
        s += f * f;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------
// finalize of optimizer.hip, the partials added in the same order, with two
// differences: grad_norm is the norm of the scaled gradient, sqrt(total) * s in
// double, and the cycle is consumed whether the step is applied or skipped
// (micro = -n). A step with nothing accumulated (micro <= 0) counts as skipped.
__global__ __launch_bounds__(1024) void finalize_main(const float* __restrict__ partials, long nparts, float max_norm,
                                                      float beta1, float beta2, int average,
                                                      State* __restrict__ state) {
  __shared__ double red[16];
  double s = 0.0;
  for (long i = threadIdx.x; i < nparts; i += 1024) s += (double)partials[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = red[0];
  for (int q = 1; q < 16; ++q) total += red[q];
  const int n = state->micro;
  if (n > 0) state->micro = -n;
  float clip = 1.f;
  bool skip = n <= 0;
  if (!skip && nparts > 0) {
    const double scale = average ? 1.0 / (double)n : 1.0;
    const float norm = (float)(sqrt(total) * scale);
    state->grad_norm = norm;
    skip = !(norm <= 3.4028234663852886e38f);  // inf or nan
    clip = fminf(1.f, max_norm / (norm + 1e-6f));
  }
  state->skip = skip ? 1 : 0;
  if (skip) {
    state->skipped += 1;
    return;
  }
  const int t = state->step + 1;
  state->step = t;
  state->clip = clip;
  state->bc1 = (float)(1.0 - pow((double)beta1, (double)t));
  state->bc2 = (float)(1.0 - pow((double)beta2, (double)t));
}

// ---------------------------------------------------------------------------
// adamw_step of optimizer.hip on fp32 gradients: two groups per thread and trip
// (its measured default), plain accesses, 16 independent 16-B loads in flight.
struct RegsMain {
  f32x4 g[2], p[2], m[2], v[2];
};

__device__ __forceinline__ void load8(const Row& r, const float* a, long i, RegsMain& x) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    x.g[h] = ld<false>((const f32x4*)(a + i) + h);
    x.p[h] = ld<false>((const f32x4*)(r.p + i) + h);
    x.m[h] = ld<false>((const f32x4*)(r.m + i) + h);
    x.v[h] = ld<false>((const f32x4*)(r.v + i) + h);
  }
}

__device__ __forceinline__ void step8(const Row& r, long i, const Consts& c, RegsMain& x) {
  float o[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p = x.p[h][e], m = x.m[h][e], v = x.v[h][e];
      update(c, x.g[h][e], p, m, v);
      x.p[h][e] = p;
      x.m[h][e] = m;
      x.v[h][e] = v;
      o[4 * h + e] = p;
    }
    st<false>((f32x4*)(r.p + i) + h, x.p[h]);
    st<false>((f32x4*)(r.m + i) + h, x.m[h]);
    st<false>((f32x4*)(r.v + i) + h, x.v[h]);
  }
  st<false>((bf16x8*)(r.w + i), pack_bf16x8(o, 0));
}

template <int U>
__global__ __launch_bounds__(THREADS) void adamw_step_main(const Row* __restrict__ rows, int n,
                                                           const float* __restrict__ groups,
                                                           const State* __restrict__ state, float beta1, float beta2,
                                                           float eps, int average) {
  if (state->skip) return;
  const long chunk = blockIdx.x;
  const Row r = rows[find_row(rows, n, chunk)];
  const float* a = main_of(r);
  const long off = (chunk - r.chunk0) * CHUNK;
  if (a == nullptr || off >= r.numel) return;
  const long end = r.numel - off < CHUNK ? r.numel : off + CHUNK;

  Consts c;
  {
    const int nm = -state->micro;  // finalize_main left -n
    const double scale = average && nm > 1 ? 1.0 / (double)nm : 1.0;
    const double lr = groups[2 * r.group], wd = groups[2 * r.group + 1], clip = (double)state->clip * scale;
    const double k1 = (1.0 - (double)beta1) * clip, k2 = (1.0 - (double)beta2) * clip * clip;
    c.b1 = beta1;
    c.b2 = beta2;
    c.k1h = (float)k1;
    c.k1l = (float)(k1 - (double)c.k1h);
    c.k2h = (float)k2;
    c.k2l = (float)(k2 - (double)c.k2h);
    c.decay = (float)(1.0 - lr * wd);
    c.lr = (float)lr;
    c.bc1 = state->bc1;
    c.bc2 = state->bc2;
    c.eps = eps;
  }

  long i = off + 8L * threadIdx.x;
  if constexpr (U == 2) {
    for (; i + SPAN + 8 <= end; i += 2 * SPAN) {
      RegsMain x, y;
      load8(r, a, i, x);
      load8(r, a, i + SPAN, y);
      step8(r, i, c, x);
      step8(r, i + SPAN, c, y);
    }
  }
  for (; i + 8 <= end; i += SPAN) {
    RegsMain x;
    load8(r, a, i, x);
    step8(r, i, c, x);
  }
  if (i < end) {
    for (; i < end; ++i) {
      float p = ld<false>(r.p + i), m = ld<false>(r.m + i), v = ld<false>(r.v + i);
      update(c, ld<false>(a + i), p, m, v);
      st<false>(r.p + i, p);
      st<false>(r.m + i, m);
      st<false>(r.v + i, v);
      st<false>(r.w + i, f2bf(p));
    }
  }
}

}  // namespace opt
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline int table_args(int ntensors, long nchunks) {
  if (ntensors < 0 || nchunks < 0 || nchunks > 0x7fffffffL || (nchunks > 0 && ntensors == 0)) return KGS_ERR_SHAPE;
  return 0;
}

// The HOST copies of the two tables grad_accumulate takes, each already through
// kgs_adamw_table_check: row for row the same numel, group and chunk0, and a main
// gradient for every tensor that has elements (the kernel writes it even when the
// bf16 gradient is missing). Returns 0, KGS_ERR_SHAPE or KGS_ERR_ALIGN.
KGS_EXPORT int kgs_grad_accum_table_check(const void* host_grad_rows, const void* host_main_rows, int ntensors) {
  if (ntensors < 0 || (ntensors > 0 && (!host_grad_rows || !host_main_rows))) return KGS_ERR_SHAPE;
  const kgs::opt::Row* g = (const kgs::opt::Row*)host_grad_rows;
  const kgs::opt::Row* m = (const kgs::opt::Row*)host_main_rows;
  for (int t = 0; t < ntensors; ++t) {
    if (g[t].numel < 0 || g[t].numel != m[t].numel || g[t].group != m[t].group || g[t].chunk0 != m[t].chunk0)
      return KGS_ERR_SHAPE;
    if (!al16(g[t].g) || !al16(m[t].g) || (m[t].numel > 0 && !m[t].g)) return KGS_ERR_ALIGN;
  }
  return 0;
}

// One micro-batch into the main gradients of every tensor, then the count: two
// launches (the count alone when there are no chunks). zero_grads: the bf16
// gradients are left as zero bits.
KGS_EXPORT int kgs_grad_accumulate(const void* grad_table, const void* main_table, int ntensors, long nchunks,
                                   void* state, int zero_grads, hipStream_t s) {
  if (const int rc = table_args(ntensors, nchunks)) return rc;
  if (!state || !al16(state)) return KGS_ERR_ALIGN;
  if (nchunks > 0 && (!grad_table || !main_table || !al16(grad_table) || !al16(main_table))) return KGS_ERR_ALIGN;
  using namespace kgs::opt;
  if (nchunks > 0) {
    const dim3 g((unsigned)nchunks), b(THREADS);
    auto G = (const Row*)grad_table;
    auto M = (const Row*)main_table;
    if (zero_grads) hipLaunchKernelGGL(grad_accumulate<true>, g, b, 0, s, G, M, ntensors, (const State*)state);
    else hipLaunchKernelGGL(grad_accumulate<false>, g, b, 0, s, G, M, ntensors, (const State*)state);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(micro_advance, dim3(1), dim3(64), 0, s, (State*)state);
  return (int)hipGetLastError();
}

// partials[c] = sum of squares of the main-gradient elements of chunk c (0 for a
// tensor whose row has no main gradient).
KGS_EXPORT int kgs_main_sumsq(const void* main_table, int ntensors, long nchunks, float* partials, hipStream_t s) {
  if (const int rc = table_args(ntensors, nchunks)) return rc;
  if (nchunks == 0) return 0;
  if (!main_table || !partials || !al16(main_table) || ((uintptr_t)partials & 3)) return KGS_ERR_ALIGN;
  using namespace kgs::opt;
  hipLaunchKernelGGL(main_sumsq<true>, dim3((unsigned)nchunks), dim3(THREADS), 0, s, (const Row*)main_table, ntensors,
                     partials);
  return (int)hipGetLastError();
}

// kgs_adamw_finalize for a main-gradient step: grad_norm and clip are those of
// s * main, s = 1 / micro for `average` and 1 otherwise; the cycle is consumed.
// Always one launch.
KGS_EXPORT int kgs_main_finalize(const float* partials, long nparts, float max_norm, float beta1, float beta2,
                                 int average, void* state, hipStream_t s) {
  if (nparts < 0) return KGS_ERR_SHAPE;
  if (!state || !al16(state) || (nparts > 0 && (!partials || ((uintptr_t)partials & 3)))) return KGS_ERR_ALIGN;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || (nparts > 0 && !(max_norm > 0.f)))
    return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::opt::finalize_main, dim3(1), dim3(1024), 0, s, partials, nparts, max_norm, beta1, beta2,
                     average, (kgs::opt::State*)state);
  return (int)hipGetLastError();
}

// kgs_adamw_step on the main table: every tensor whose row has a main gradient.
KGS_EXPORT int kgs_adamw_step_main(const void* main_table, int ntensors, long nchunks, const float* groups,
                                   const void* state, float beta1, float beta2, float eps, int average,
                                   hipStream_t s) {
  if (const int rc = table_args(ntensors, nchunks)) return rc;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return KGS_ERR_ARG;
  if (nchunks == 0) return 0;
  if (!main_table || !groups || !state || !al16(main_table) || !al16(state) || ((uintptr_t)groups & 7))
    return KGS_ERR_ALIGN;
  using namespace kgs::opt;
  hipLaunchKernelGGL(adamw_step_main<2>, dim3((unsigned)nchunks), dim3(THREADS), 0, s, (const Row*)main_table,
                     ntensors, groups, (const State*)state, beta1, beta2, eps, average);
  return (int)hipGetLastError();
}
