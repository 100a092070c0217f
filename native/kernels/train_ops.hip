// Training glue for gfx950: the backward passes of the memory-bound ops of a
// Llama layer and the softmax cross-entropy over the LM head's logits.
//
//   * rmsnorm_bwd   : dx and dw of y = rmsnorm(x) * w, with the gradient that
//                     reaches x through the residual branch added before the
//                     one rounding of dx
//   * silu_mul_bwd  : d(gate|up) of h = silu(gate) * up, in the fused layout
//   * xent_fwd/_bwd : per-row log-sum-exp and loss = lse - x[target]; dlogits =
//                     grow * (softmax - onehot)
//
// The backward of rope_qkv is rope_qkv itself with the negated sin table
// (transformer.hip): the transposed rotation, no kernel here.
//
// House rules (attention_train.hip): fp32 math, one bf16 rounding per output
// element, 16-B accesses, no float atomics, no workgroup waits on another. Every
// result is a function of the inputs and the shape only: the grids and the
// summation orders below are computed from the shape, never from an occupancy
// query, so every kernel is bitwise repeatable and capturable in a hipGraph.
#include "kgs_common.h"

namespace kgs {
namespace trn {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// ---------------------------------------------------------------------------
// RMSNorm backward. Stage 1: one wave per row with add_rmsnorm's lane-to-column
// ownership (lane owns the 16-B chunks lane + 64 j, cols == 512 NC), so a lane
// adds to the same dw columns on every row while its wave walks rows wave,
// wave + W, wave + 2 W, ... (W = 4 * gridDim.x, the grid capped at NORM_BWD_WGS
// workgroups). The fp32 dw accumulators of a wave live in its own 2 NC KiB of
// LDS, not in registers: at NC = 16 they would be 128 VGPRs next to the row's
// x and dy (kept packed as bf16, 128 more), before any operand is unpacked.
// A lane reads and writes only its own LDS words, so the row loop needs no
// barrier. After the loop the four waves' rows are added in wave order and the
// workgroup stores ONE fp32 partial row; stage 2 sums the partial rows.
constexpr int NORM_BWD_WGS = 512;

template <int NC>
__global__ __launch_bounds__(256) void rmsnorm_bwd(const unsigned short* __restrict__ x,
                                                   const unsigned short* __restrict__ w,
                                                   const unsigned short* __restrict__ dy,
                                                   const unsigned short* __restrict__ dres,
                                                   unsigned short* __restrict__ dx, float* __restrict__ ws, int rows,
                                                   long ldx, long lddy, long lddres, long lddx, float eps) {
  constexpr int WV = 2 * 64 * NC;  // f32x4 words of one wave's accumulator row: [j][half][lane]
  __shared__ f32x4 acc[4 * WV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nwaves = 4L * gridDim.x;
  const bf16x8* wr = (const bf16x8*)w;
  constexpr float inv_cols = 1.f / (float)(NC * 512);
  f32x4* mine = acc + wave * WV + lane;
#pragma unroll
  for (int q = 0; q < 2 * NC; ++q) mine[64 * q] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (long row = 4L * blockIdx.x + wave; row < rows; row += nwaves) {
    const bf16x8* xr = (const bf16x8*)(x + row * ldx);
    const bf16x8* gr = (const bf16x8*)(dy + row * lddy);
    bf16x8 xv[NC], gv[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) xv[j] = __builtin_nontemporal_load(xr + lane + 64 * j);
#pragma unroll
    for (int j = 0; j < NC; ++j) gv[j] = __builtin_nontemporal_load(gr + lane + 64 * j);
    float ss = 0.f, cs = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const bf16x8 wv = wr[lane + 64 * j];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf2f((unsigned short)xv[j][e]);
        const float g = bf2f((unsigned short)gv[j][e]) * bf2f((unsigned short)wv[e]);
        ss += xf * xf;
        cs += g * xf;
      }
    }
    ss = wave_sum(ss);
    cs = wave_sum(cs);
    const float r = rsqrtf(ss * inv_cols + eps);
    const float k = r * r * r * (cs * inv_cols);
    bf16x8* or_ = (bf16x8*)(dx + row * lddx);
    // the second pass unpacks x and dy again: without this fence hipcc keeps the
    // first pass's fp32 copies alive across the row sums (16 NC VGPRs)
#pragma unroll
    for (int j = 0; j < NC; ++j) asm volatile("" : "+v"(xv[j]), "+v"(gv[j]));
    const bf16x8* rr = dres != nullptr ? (const bf16x8*)(dres + row * lddres) : nullptr;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const bf16x8 wv = wr[lane + 64 * j];  // again, from L1: kept, it would be 4 NC more VGPRs
      bf16x8 rv;
      if (dres != nullptr) rv = __builtin_nontemporal_load(rr + lane + 64 * j);
      float o[8], a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf2f((unsigned short)xv[j][e]);
        const float df = bf2f((unsigned short)gv[j][e]);
        float t = r * (df * bf2f((unsigned short)wv[e])) - xf * k;
        if (dres != nullptr) t += bf2f((unsigned short)rv[e]);
        o[e] = t;
        a[e] = (df * xf) * r;
      }
      or_[lane + 64 * j] = pack_bf16x8(o, 0);
      mine[64 * (2 * j)] += f32x4{a[0], a[1], a[2], a[3]};
      mine[64 * (2 * j + 1)] += f32x4{a[4], a[5], a[6], a[7]};
    }
  }

  // the workgroup's partial row: wave 0 + wave 1 + wave 2 + wave 3, in that order
  __syncthreads();
  f32x4* out = (f32x4*)(ws + (long)blockIdx.x * (NC * 512));
  for (int i = threadIdx.x; i < WV; i += 256) {
    const int l = i & 63, half = (i >> 6) & 1, j = i >> 7;
    out[2 * (l + 64 * j) + half] = ((acc[i] + acc[WV + i]) + acc[2 * WV + i]) + acc[3 * WV + i];
  }
}

// Stage 2: dw[c] = bf16(sum over the nparts partial rows). A workgroup owns 64
// columns; thread (oct, grp) = (t & 7, t >> 3) sums the partial rows grp * per
// .. (grp + 1) * per - 1 of column octet oct in index order, then the 32 group
// sums are added in group order through LDS: one fixed tree per (nparts, cols).
__global__ __launch_bounds__(256) void rmsnorm_bwd_dw(const float* __restrict__ ws, unsigned short* __restrict__ dw,
                                                      int nparts, int cols) {
  __shared__ f32x4 red[32][2][8];
  const int oct = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const long c8 = 8L * blockIdx.x + oct;  // this thread's column octet
  const int per = (nparts + 31) / 32;
  const int p1 = min(nparts, (grp + 1) * per);
  f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
  for (int p = grp * per; p < p1; ++p) {
    const f32x4* pr = (const f32x4*)(ws + (long)p * cols) + 2 * c8;
    lo += pr[0];
    hi += pr[1];
  }
  red[grp][0][oct] = lo;
  red[grp][1][oct] = hi;
  __syncthreads();
  if (grp == 0) {
    for (int q = 1; q < 32; ++q) {
      lo += red[q][0][oct];
      hi += red[q][1][oct];
    }
    const float o[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    ((bf16x8*)dw)[c8] = pack_bf16x8(o, 0);
  }
}

// ---------------------------------------------------------------------------
// SwiGLU backward: thread = one 8-wide chunk of gate and the matching chunk of
// up (silu_mul's mapping). With s = sigmoid(g):
//   dgate = dh * u * s * (1 + g * (1 - s)),   dup = dh * g * s.
// The trailing + 0 turns a -0 product into +0: dh = 0 gives zero bits.
__global__ __launch_bounds__(256) void silu_mul_bwd(const unsigned short* __restrict__ gu,
                                                    const unsigned short* __restrict__ dh,
                                                    unsigned short* __restrict__ dgu, long rows, int inter, long ld_gu,
                                                    long ld_dh, long ld_dgu) {
  const int cpr = inter / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * cpr) return;
  const long r = idx / cpr;
  const int c = (int)(idx - r * cpr);
  const bf16x8 g = __builtin_nontemporal_load((const bf16x8*)(gu + r * ld_gu) + c);
  const bf16x8 u = __builtin_nontemporal_load((const bf16x8*)(gu + r * ld_gu + inter) + c);
  const bf16x8 d = __builtin_nontemporal_load((const bf16x8*)(dh + r * ld_dh) + c);
  float og[8], ou[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float gf = bf2f((unsigned short)g[e]), uf = bf2f((unsigned short)u[e]), df = bf2f((unsigned short)d[e]);
    const float s = 1.0f / (1.0f + __expf(-gf));
    og[e] = df * uf * s * (1.0f + gf * (1.0f - s)) + 0.0f;
    ou[e] = df * gf * s + 0.0f;
  }
  ((bf16x8*)(dgu + r * ld_dgu))[c] = pack_bf16x8(og, 0);
  ((bf16x8*)(dgu + r * ld_dgu + inter))[c] = pack_bf16x8(ou, 0);
}

// ---------------------------------------------------------------------------
// Softmax cross-entropy forward: one 1024-thread workgroup per row, ONE pass
// over the row. A thread keeps a running maximum m and the sum s of exp(x - m),
// rescaled whenever m grows (once per batch of eight 16-B loads, which are all
// issued before the first use, as in argmax_rows); the pairs are then merged
// through the wave and an LDS tree. lse = m + log(s), loss = lse - x[target];
// a target outside [0, cols) makes the row ignored (loss 0, lse still written).
constexpr float XENT_FLOOR = -3.0e38f;  // a finite "-inf": exp(x - m) never sees inf - inf

__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mn = fmaxf(m, om);
  s = s * exp2f((m - mn) * LOG2E) + os * exp2f((om - mn) * LOG2E);
  m = mn;
}

__global__ __launch_bounds__(1024) void xent_fwd(const unsigned short* __restrict__ x,
                                                 const long long* __restrict__ target, float* __restrict__ loss,
                                                 float* __restrict__ lse, int cols, long ld) {
  __shared__ float sm[16], ssum[16];
  const long row = blockIdx.x;
  const int t = threadIdx.x;
  const bf16x8* xr = (const bf16x8*)(x + row * ld);
  const int nch = cols / 8;
  float m = XENT_FLOOR, s = 0.f;
  for (int c0 = t; c0 < nch; c0 += 1024 * 8) {
    bf16x8 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __builtin_nontemporal_load(xr + min(c0 + 1024 * j, nch - 1));
    float bm = XENT_FLOOR;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c0 + 1024 * j < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bm = fmaxf(bm, bf2f((unsigned short)v[j][e]));
      }
    }
    const float mn = fmaxf(m, bm);
    float bs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c0 + 1024 * j < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bs += exp2f((bf2f((unsigned short)v[j][e]) - mn) * LOG2E);
      }
    }
    s = s * exp2f((m - mn) * LOG2E) + bs;
    m = mn;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    lse_merge(m, s, om, os);
  }
  if ((t & 63) == 0) {
    sm[t >> 6] = m;
    ssum[t >> 6] = s;
  }
  __syncthreads();
  if (t < 64) {
    m = t < 16 ? sm[t] : XENT_FLOOR;
    s = t < 16 ? ssum[t] : 0.f;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
      lse_merge(m, s, om, os);
    }
    if (t == 0) {
      const float l = m + __log2f(s) * LN2;
      const long long tg = target[row];
      const bool live = tg >= 0 && tg < cols;
      lse[row] = l;
      loss[row] = live ? l - bf2f(x[row * ld + (live ? tg : 0)]) : 0.f;
    }
  }
}

// dlogits = bf16(grow * (exp(x - lse) - [col == target])); an ignored row is
// written as zeros. One 1024-thread workgroup per row, two passes over it (the
// second finds the row in L2). At the target, p - 1 cancels: a peaky row has p
// = 1 in fp32 and would get a zero there while the other columns keep their
// e^-60, so the row would no longer sum to zero. The first pass therefore sums
// the OTHER columns' p (wave sums, then the 16 waves in index order) and the
// target gets -grow * that sum: the same quantity without the cancellation.
// The trailing + 0 keeps a zero product's sign positive (grow = 0: zero bits).
__global__ __launch_bounds__(1024) void xent_bwd(const unsigned short* __restrict__ x,
                                                 const long long* __restrict__ target,
                                                 const float* __restrict__ lse, const float* __restrict__ grow,
                                                 unsigned short* __restrict__ dl, int cols, long ld, long ldd) {
  __shared__ float red[16];
  const long row = blockIdx.x;
  const int t = threadIdx.x, nch = cols / 8;
  const long long tg = target[row];
  bf16x8* out = (bf16x8*)(dl + row * ldd);
  if (tg < 0 || tg >= cols) {
    for (int c = t; c < nch; c += 1024) out[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    return;
  }
  const bf16x8* xr = (const bf16x8*)(x + row * ld);
  const float l = lse[row], g = grow[row];
  const int tc = (int)tg >> 3, te = (int)tg & 7;  // the target's chunk and element
  float rest = 0.f;
  for (int c0 = t; c0 < nch; c0 += 1024 * 8) {
    bf16x8 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = xr[min(c0 + 1024 * j, nch - 1)];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + 1024 * j;
      if (c < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float p = exp2f((bf2f((unsigned short)v[j][e]) - l) * LOG2E);
          rest += (c == tc && e == te) ? 0.f : p;
        }
      }
    }
  }
  rest = wave_sum(rest);
  if ((t & 63) == 0) red[t >> 6] = rest;
  __syncthreads();
  rest = red[0];
#pragma unroll
  for (int q = 1; q < 16; ++q) rest += red[q];
  for (int c0 = t; c0 < nch; c0 += 1024 * 8) {
    bf16x8 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __builtin_nontemporal_load(xr + min(c0 + 1024 * j, nch - 1));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + 1024 * j;
      if (c < nch) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float p = exp2f((bf2f((unsigned short)v[j][e]) - l) * LOG2E);
          o[e] = g * ((c == tc && e == te) ? -rest : p) + 0.0f;
        }
        out[c] = pack_bf16x8(o, 0);
      }
    }
  }
}

}  // namespace trn
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline int norm_bwd_parts(int rows) {
  const long wgs = ((long)rows + 3) / 4;
  return (int)(wgs < kgs::trn::NORM_BWD_WGS ? wgs : kgs::trn::NORM_BWD_WGS);
}

// Bytes of the fp32 workspace kgs_rmsnorm_bwd_bf16 needs (one partial dw row per
// stage-1 workgroup), or KGS_ERR_SHAPE. At least 16, so there is always a buffer.
KGS_EXPORT long kgs_rmsnorm_bwd_workspace(int rows, int cols) {
  if (rows < 0 || cols <= 0 || cols % 512 || cols > 8192) return KGS_ERR_SHAPE;
  const long b = (long)norm_bwd_parts(rows) * cols * 4;
  return b < 16 ? 16 : b;
}

// x: [rows, ldx] the stream value the forward normalised (x + d as add_rmsnorm
// wrote it back); w: [cols]; dy: [rows, lddy]; dres: optional [rows, lddres],
// the gradient reaching the same stream value through the residual branch.
// dx: [rows, lddx] = bf16(dres + r g - x r^3 c); dw: [cols]. ws: fp32 workspace
// of kgs_rmsnorm_bwd_workspace(rows, cols) bytes. Two launches, nothing
// allocated, nothing synchronised.
KGS_EXPORT int kgs_rmsnorm_bwd_bf16(const void* x, const void* w, const void* dy, const void* dres, void* dx, void* dw,
                                   void* ws, int rows, int cols, long ldx, long lddy, long lddres, long lddx,
                                   float eps, hipStream_t s) {
  if (rows < 0 || cols <= 0) return KGS_ERR_SHAPE;
  if (cols % 512 || cols > 8192 || ldx < cols || lddy < cols || lddx < cols || (dres && lddres < cols))
    return KGS_ERR_SHAPE;
  if (!x || !w || !dy || !dx || !dw || !ws) return KGS_ERR_ALIGN;
  if (!al16(x) || !al16(w) || !al16(dy) || !al16(dres) || !al16(dx) || !al16(dw) || !al16(ws)) return KGS_ERR_ALIGN;
  if (ldx % 8 || lddy % 8 || lddx % 8 || (dres && lddres % 8)) return KGS_ERR_ALIGN;
  using namespace kgs::trn;
  const int parts = norm_bwd_parts(rows);
  auto X = (const unsigned short*)x;
  auto W = (const unsigned short*)w;
  auto G = (const unsigned short*)dy;
  auto R = (const unsigned short*)dres;
  auto DX = (unsigned short*)dx;
  auto WS = (float*)ws;
  if (parts > 0) {
    const dim3 g(parts), b(256);
    switch (cols / 512) {
#define KGS_NC(n) \
  case n: hipLaunchKernelGGL(rmsnorm_bwd<n>, g, b, 0, s, X, W, G, R, DX, WS, rows, ldx, lddy, lddres, lddx, eps); break;
      KGS_NC(1) KGS_NC(2) KGS_NC(3) KGS_NC(4) KGS_NC(5) KGS_NC(6) KGS_NC(7) KGS_NC(8)
      KGS_NC(9) KGS_NC(10) KGS_NC(11) KGS_NC(12) KGS_NC(13) KGS_NC(14) KGS_NC(15) KGS_NC(16)
#undef KGS_NC
      default: return KGS_ERR_SHAPE;
    }
  }
  hipLaunchKernelGGL(rmsnorm_bwd_dw, dim3(cols / 64), dim3(256), 0, s, (const float*)WS, (unsigned short*)dw, parts,
                     cols);
  return (int)hipGetLastError();
}

// gu: [rows, ld_gu] gate | up; dh: [rows, ld_dh]; dgu: [rows, ld_dgu] dgate | dup.
KGS_EXPORT int kgs_silu_mul_bwd_bf16(const void* gu, const void* dh, void* dgu, long rows, int inter, long ld_gu,
                                    long ld_dh, long ld_dgu, hipStream_t s) {
  if (rows < 0 || inter <= 0 || inter % 8 || ld_gu < 2L * inter || ld_dh < inter || ld_dgu < 2L * inter)
    return KGS_ERR_SHAPE;
  if (!gu || !dh || !dgu || !al16(gu) || !al16(dh) || !al16(dgu) || ld_gu % 8 || ld_dh % 8 || ld_dgu % 8)
    return KGS_ERR_ALIGN;
  const long n = rows * (inter / 8);
  if (n == 0) return 0;
  if ((n + 255) / 256 > 0x7fffffff) return KGS_ERR_SHAPE;
  hipLaunchKernelGGL(kgs::trn::silu_mul_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     (const unsigned short*)gu, (const unsigned short*)dh, (unsigned short*)dgu, rows, inter, ld_gu,
                     ld_dh, ld_dgu);
  return (int)hipGetLastError();
}

// logits: [rows, ld] bf16 (cols % 8 == 0); target: int64 [rows]; loss, lse: fp32 [rows].
KGS_EXPORT int kgs_xent_fwd_bf16(const void* logits, const void* target, float* loss, float* lse, int rows, int cols,
                                long ld, hipStream_t s) {
  if (rows < 0 || cols <= 0 || cols % 8 || ld < cols) return KGS_ERR_SHAPE;
  if (!logits || !target || !loss || !lse || !al16(logits) || ld % 8) return KGS_ERR_ALIGN;
  if (((uintptr_t)target & 7) || ((uintptr_t)loss & 3) || ((uintptr_t)lse & 3)) return KGS_ERR_ALIGN;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(kgs::trn::xent_fwd, dim3(rows), dim3(1024), 0, s, (const unsigned short*)logits,
                     (const long long*)target, loss, lse, cols, ld);
  return (int)hipGetLastError();
}

// dlogits: [rows, ldd] bf16, a buffer of its own; grow: fp32 [rows], the
// upstream gradient of each row's loss. Only columns < cols are written.
KGS_EXPORT int kgs_xent_bwd_bf16(const void* logits, const void* target, const float* lse, const float* grow,
                                void* dlogits, int rows, int cols, long ld, long ldd, hipStream_t s) {
  if (rows < 0 || cols <= 0 || cols % 8 || ld < cols || ldd < cols) return KGS_ERR_SHAPE;
  if (!logits || !target || !lse || !grow || !dlogits || !al16(logits) || !al16(dlogits) || ld % 8 || ldd % 8)
    return KGS_ERR_ALIGN;
  if (((uintptr_t)target & 7) || ((uintptr_t)lse & 3) || ((uintptr_t)grow & 3)) return KGS_ERR_ALIGN;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(kgs::trn::xent_bwd, dim3(rows), dim3(1024), 0, s, (const unsigned short*)logits,
                     (const long long*)target, lse, grow, (unsigned short*)dlogits, cols, ld, ldd);
  return (int)hipGetLastError();
}
