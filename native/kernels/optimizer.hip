// Fused AdamW for gfx950: fp32 master weights and moments, the bf16 weights
// re-rounded from the master, global-norm gradient clipping, every tensor of a
// model in three launches and no host synchronisation.
//
//   * grad_sumsq : one fp32 sum of squares of the bf16 gradients per work chunk
//   * finalize   : one workgroup; partials -> grad_norm, clip, the skip decision,
//                  the step counter and the bias corrections
//   * adamw_step : per element, in fp32,
//                    g = clip * float(g_bf16)
//                    m = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g^2
//                    p = p (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps)
//                  p, m, v stored as fp32, the bf16 weight = RNE(stored p)
//
// Device-resident arguments (kgs/ops/optim.py builds them):
//
//   tensor table, one 64-byte row per tensor, eight 64-bit words:
//     0 w      bf16 weight                 4 g      bf16 gradient, 0 = no gradient
//     1 p      fp32 master                          this step: the tensor is skipped
//     2 m      fp32 first moment           5 numel  >= 0
//     3 v      fp32 second moment          6 group  row of the group block
//                                          7 chunk0 work chunks before this tensor
//     A chunk is KGS_ADAMW_CHUNK consecutive elements of ONE tensor; tensor t owns
//     the chunks chunk0[t] .. chunk0[t] + ceil(numel / CHUNK) - 1, its last one
//     the tail of any length. Every pointer is 16-byte aligned
//     (kgs_adamw_table_check, on the host copy, before the table is uploaded).
//   group block: float {lr, weight_decay} per group.
//   state block, eight 32-bit words:
//     0 step (int)  1 skipped (int)  2 grad_norm  3 clip  4 bc1 = 1 - b1^step
//     5 bc2 = 1 - b2^step  6 skip flag of the current step (int)
//     7 micro-batch count of grad_accum.hip (int), untouched by this file
//
// lr, the step counter and the clip factor live on the device so that a captured
// step replays with new values: nothing of them is baked into a kernel argument.
//
// A workgroup owns one chunk and finds its tensor by a binary search over
// chunk0 on its (wave-uniform) block index. Every sum has an order fixed by the
// shape: in-lane, wave, workgroup, then the partials in index order; no atomics.
//
// House rules (train_ops.hip): 16-B accesses, no allocation or synchronisation
// in an entry, nothing launched for empty work.
#include "optimizer_common.h"

namespace kgs {
namespace opt {

// the __global__ functions of this file, template instantiations counted once
// each (tests/test_optim.py compares it with what the compiler reports)
constexpr int KERNEL_COUNT = 9;

// ---------------------------------------------------------------------------
// One partial per chunk. A thread owns the 16-B groups tid, tid + 256, ... of
// the chunk (CHUNK / SPAN = 8 of them, all loaded before the first use) and
// adds their squares in element order; the chunk's last, shorter group is
// read element by element by the one thread that owns it.
template <bool NT>
__global__ __launch_bounds__(THREADS) void grad_sumsq(const Row* __restrict__ rows, int n,
                                                      float* __restrict__ partials) {
  __shared__ float red[THREADS / 64];
  const long chunk = blockIdx.x;
  const Row r = rows[find_row(rows, n, chunk)];
  const long off = (chunk - r.chunk0) * CHUNK;
  float s = 0.f;
  if (r.g != nullptr && off < r.numel) {
    const long end = r.numel - off < CHUNK ? r.numel : off + CHUNK;
    const long i0 = off + 8L * threadIdx.x;
    constexpr int T = CHUNK / SPAN;
    bf16x8 gv[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const long i = i0 + (long)j * SPAN;
      gv[j] = i + 8 <= end ? ld<NT>((const bf16x8*)(r.g + i)) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf2f((unsigned short)gv[j][e]);
        s += f * f;
      }
    }
    const long t0 = end & ~7L;  // the short group, if any, starts here
    if (t0 < end && (int)(((t0 - off) >> 3) % THREADS) == (int)threadIdx.x) {
      for (long i = t0; i < end; ++i) {
        const float f = bf2f(ld<false>(r.g + i));
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
// One workgroup. Thread t adds the partials t, t + 1024, ... in index order, in
// double; then the wave, then the 16 waves in wave order. nparts == 0: clipping
// is off, clip = 1 and the step is never skipped (grad_norm is left alone).
__global__ __launch_bounds__(1024) void finalize(const float* __restrict__ partials, long nparts, float max_norm,
                                                 float beta1, float beta2, State* __restrict__ state) {
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
  float clip = 1.f;
  bool skip = false;
  if (nparts > 0) {
    const float norm = (float)sqrt(total);
    state->grad_norm = norm;
    skip = !(norm <= 3.4028234663852886e38f);  // inf or nan
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
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
  // in double: 1 - b2^t loses most of its digits in fp32 while t is small
  state->bc1 = (float)(1.0 - pow((double)beta1, (double)t));
  state->bc2 = (float)(1.0 - pow((double)beta2, (double)t));
}

// ---------------------------------------------------------------------------
// The update of one element, its constants and their error analysis:
// optimizer_common.h (Consts, update).
struct Regs {
  bf16x8 g;
  f32x4 p[2], m[2], v[2];
};

template <bool NTL>
__device__ __forceinline__ void load8(const Row& r, long i, Regs& x) {
  x.g = ld<NTL>((const bf16x8*)(r.g + i));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    x.p[h] = ld<NTL>((const f32x4*)(r.p + i) + h);
    x.m[h] = ld<NTL>((const f32x4*)(r.m + i) + h);
    x.v[h] = ld<NTL>((const f32x4*)(r.v + i) + h);
  }
}

template <bool NT>
__device__ __forceinline__ void step8(const Row& r, long i, const Consts& c, Regs& x) {
  float o[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p = x.p[h][e], m = x.m[h][e], v = x.v[h][e];
      update(c, bf2f((unsigned short)x.g[4 * h + e]), p, m, v);
      x.p[h][e] = p;
      x.m[h][e] = m;
      x.v[h][e] = v;
      o[4 * h + e] = p;
    }
    st<NT>((f32x4*)(r.p + i) + h, x.p[h]);
    st<NT>((f32x4*)(r.m + i) + h, x.m[h]);
    st<NT>((f32x4*)(r.v + i) + h, x.v[h]);
  }
  st<NT>((bf16x8*)(r.w + i), pack_bf16x8(o, 0));
}

// U 16-B groups per thread and trip: 7 U independent 16-B loads are issued
// before the first use. The chunk's short last group (numel % 8 elements) is
// done element by element by the thread that owns it: nothing past numel is
// read or written. NTL / NTS: non-temporal loads / stores.
template <bool NTL, bool NTS, int U>
__global__ __launch_bounds__(THREADS) void adamw_step(const Row* __restrict__ rows, int n,
                                                      const float* __restrict__ groups,
                                                      const State* __restrict__ state, float beta1, float beta2,
                                                      float eps) {
  if (state->skip) return;
  const long chunk = blockIdx.x;
  const Row r = rows[find_row(rows, n, chunk)];
  const long off = (chunk - r.chunk0) * CHUNK;
  if (r.g == nullptr || off >= r.numel) return;
  const long end = r.numel - off < CHUNK ? r.numel : off + CHUNK;

  Consts c;
  {
    const double lr = groups[2 * r.group], wd = groups[2 * r.group + 1], clip = state->clip;
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
      Regs a, b;
      load8<NTL>(r, i, a);
      load8<NTL>(r, i + SPAN, b);
      step8<NTS>(r, i, c, a);
      step8<NTS>(r, i + SPAN, c, b);
    }
  }
  for (; i + 8 <= end; i += SPAN) {
    Regs a;
    load8<NTL>(r, i, a);
    step8<NTS>(r, i, c, a);
  }
  if (i < end) {
    for (; i < end; ++i) {
      float p = ld<false>(r.p + i), m = ld<false>(r.m + i), v = ld<false>(r.v + i);
      update(c, bf2f(ld<false>(r.g + i)), p, m, v);
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

// Streaming variants. adamw_step: 0 plain, 1 non-temporal loads and stores, 2 and 3
// the same with two 16-B groups per thread and trip, 4 two groups with non-temporal
// loads only, 5 two groups with non-temporal stores only. grad_sumsq: odd = non-
// temporal loads. The defaults are the measured best of each kernel
// (profiles/r13/optimizer/README.md): the update streams fastest with plain
// accesses and two groups, the norm pass with non-temporal loads.
#define KGS_ADAMW_VARIANTS 6
#define KGS_ADAMW_STEP_DEFAULT 2
#define KGS_ADAMW_SUMSQ_DEFAULT 1

KGS_EXPORT int kgs_adamw_chunk(void) { return KGS_ADAMW_CHUNK; }
KGS_EXPORT int kgs_adamw_row_bytes(void) { return (int)sizeof(kgs::opt::Row); }
KGS_EXPORT int kgs_adamw_state_bytes(void) { return (int)sizeof(kgs::opt::State); }
KGS_EXPORT int kgs_adamw_step_default_variant(void) { return KGS_ADAMW_STEP_DEFAULT; }
KGS_EXPORT int kgs_adamw_sumsq_default_variant(void) { return KGS_ADAMW_SUMSQ_DEFAULT; }

// The HOST copy of a tensor table, before it is uploaded: the kernels trust the
// device table. Returns the number of work chunks, or KGS_ERR_ALIGN for a null
// (unless numel is 0) or misaligned w / p / m / v or a misaligned g, KGS_ERR_SHAPE for a negative numel
// or a chunk0 that is not the running sum of ceil(numel / CHUNK), KGS_ERR_ARG for
// a group outside [0, ngroups).
KGS_EXPORT long kgs_adamw_table_check(const void* host_rows, int ntensors, int ngroups) {
  if (ntensors < 0 || ngroups < 0 || (ntensors > 0 && !host_rows)) return KGS_ERR_SHAPE;
  const kgs::opt::Row* rows = (const kgs::opt::Row*)host_rows;
  long chunks = 0;
  for (int t = 0; t < ntensors; ++t) {
    const kgs::opt::Row& r = rows[t];
    if (r.numel < 0 || r.chunk0 != chunks) return KGS_ERR_SHAPE;
    if (r.group < 0 || r.group >= ngroups) return KGS_ERR_ARG;
    if (r.numel > 0 && (!r.w || !r.p || !r.m || !r.v)) return KGS_ERR_ALIGN;
    if (!al16(r.w) || !al16(r.p) || !al16(r.m) || !al16(r.v) || !al16(r.g)) return KGS_ERR_ALIGN;
    chunks += (r.numel + KGS_ADAMW_CHUNK - 1) / KGS_ADAMW_CHUNK;
    if (chunks > 0x7fffffffL) return KGS_ERR_SHAPE;
  }
  return chunks;
}

// partials[c] = sum of squares of the gradient elements of chunk c (0 for a tensor
// without a gradient), c < nchunks = what kgs_adamw_table_check returned.
KGS_EXPORT int kgs_adamw_grad_sumsq_v(const void* table, int ntensors, long nchunks, float* partials, int variant,
                                      hipStream_t s) {
  if (ntensors < 0 || nchunks < 0 || nchunks > 0x7fffffffL || (nchunks > 0 && ntensors == 0)) return KGS_ERR_SHAPE;
  if (variant < 0 || variant >= KGS_ADAMW_VARIANTS) return KGS_ERR_ARG;
  if (nchunks == 0) return 0;
  if (!table || !partials || !al16(table) || ((uintptr_t)partials & 3)) return KGS_ERR_ALIGN;
  using namespace kgs::opt;
  const dim3 g((unsigned)nchunks), b(THREADS);
  if (variant & 1) hipLaunchKernelGGL(grad_sumsq<true>, g, b, 0, s, (const Row*)table, ntensors, partials);
  else hipLaunchKernelGGL(grad_sumsq<false>, g, b, 0, s, (const Row*)table, ntensors, partials);
  return (int)hipGetLastError();
}

KGS_EXPORT int kgs_adamw_grad_sumsq(const void* table, int ntensors, long nchunks, float* partials, hipStream_t s) {
  return kgs_adamw_grad_sumsq_v(table, ntensors, nchunks, partials, KGS_ADAMW_SUMSQ_DEFAULT, s);
}

// The step's scalar work. nparts > 0: grad_norm = sqrt(sum of the partials), clip =
// min(1, max_norm / (grad_norm + 1e-6)); a grad_norm that is not finite sets the
// skip flag and counts the step in `skipped`. nparts == 0 (partials may be null):
// no clipping, clip = 1, never skipped. A step that is not skipped increments
// `step` and gets its bias corrections. Always one launch.
KGS_EXPORT int kgs_adamw_finalize(const float* partials, long nparts, float max_norm, float beta1, float beta2,
                                  void* state, hipStream_t s) {
  if (nparts < 0) return KGS_ERR_SHAPE;
  if (!state || !al16(state) || (nparts > 0 && (!partials || ((uintptr_t)partials & 3)))) return KGS_ERR_ALIGN;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || (nparts > 0 && !(max_norm > 0.f)))
    return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::opt::finalize, dim3(1), dim3(1024), 0, s, partials, nparts, max_norm, beta1, beta2,
                     (kgs::opt::State*)state);
  return (int)hipGetLastError();
}

// The update of every tensor of the table that has a gradient, with the clip,
// step and bias corrections kgs_adamw_finalize left in the state block and the
// groups' {lr, weight_decay} read from the device.
KGS_EXPORT int kgs_adamw_step_v(const void* table, int ntensors, long nchunks, const float* groups, const void* state,
                                float beta1, float beta2, float eps, int variant, hipStream_t s) {
  if (ntensors < 0 || nchunks < 0 || nchunks > 0x7fffffffL || (nchunks > 0 && ntensors == 0)) return KGS_ERR_SHAPE;
  if (variant < 0 || variant >= KGS_ADAMW_VARIANTS) return KGS_ERR_ARG;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return KGS_ERR_ARG;
  if (nchunks == 0) return 0;
  if (!table || !groups || !state || !al16(table) || !al16(state) || ((uintptr_t)groups & 7)) return KGS_ERR_ALIGN;
  using namespace kgs::opt;
  const dim3 g((unsigned)nchunks), b(THREADS);
  auto R = (const Row*)table;
  auto S = (const State*)state;
#define KGS_STEP(v, L, S_, U)                                                                                      \
  case v: hipLaunchKernelGGL((adamw_step<L, S_, U>), g, b, 0, s, R, ntensors, groups, S, beta1, beta2, eps); break;
  switch (variant) {
    KGS_STEP(0, false, false, 1) KGS_STEP(1, true, true, 1) KGS_STEP(2, false, false, 2)
    KGS_STEP(3, true, true, 2) KGS_STEP(4, true, false, 2) KGS_STEP(5, false, true, 2)
    default: return KGS_ERR_ARG;
  }
#undef KGS_STEP
  return (int)hipGetLastError();
}

KGS_EXPORT int kgs_adamw_step(const void* table, int ntensors, long nchunks, const float* groups, const void* state,
                              float beta1, float beta2, float eps, hipStream_t s) {
  return kgs_adamw_step_v(table, ntensors, nchunks, groups, state, beta1, beta2, eps, KGS_ADAMW_STEP_DEFAULT, s);
}
