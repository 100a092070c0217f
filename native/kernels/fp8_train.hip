// Quantising producers of the fp8 training Linear for gfx950 (OCP e4m3fn):
//
//   * fp8_amax  : ONE pass over a bf16 matrix that finds every amax an operand
//                 needs -- per row, per column and per tensor, whichever are
//                 asked for
//   * fp8_quant : ONE pass that writes the e4m3 image of the matrix and / or of
//                 its transpose, each scaled per output row or per tensor, so
//                 that all three GEMMs of a Linear (y = x w^T, dx = dy w,
//                 dw = dy^T x) stay NT on kgs_gemm_fp8_nt_rows
//
//   scale(a) = max(a, 1e-12) / 448,   q(x, s) = e4m3_rne(clamp(x * (1 / s), +-448))
//
// (quant_fp8.hip's formulas). A stored scale may carry a fold: a device scalar,
// the B operand's per-tensor scale, multiplied into the A operand's row scales
// as they are written; the quantising inverse uses the unfolded scale.
//
// Non-finite values stay visible. amax is the unsigned maximum of bits(|x|):
// NaN patterns order above Inf, Inf above every finite value, and the maximum
// is order-independent, so the atomics below give bitwise repeatable results.
// A scale whose amax is NaN or Inf is NaN or Inf (the max with 1e-12 is a
// compare-and-select, not fmaxf, which would drop the NaN); the GEMM's epilogue
// multiplies it into every output the operand row touches.
//
// House rules (train_ops.hip): 16-B global reads, no float atomics, no
// workgroup waits on another, grids computed from the shape only.
#include "kgs_common.h"

namespace kgs {
namespace f8t {

constexpr float E4M3_MAX = 448.f;
constexpr float TINY = 1e-12f;

__device__ __forceinline__ float scale_of(float amax) {
  return (amax < TINY ? TINY : amax) / E4M3_MAX;  // NaN fails the compare and stays
}

__device__ __forceinline__ float clamp448(float v) { return fminf(fmaxf(v, -E4M3_MAX), E4M3_MAX); }

// ---------------------------------------------------------------------------
// The accumulators' reset, as a kernel: captured paths use no memset node
// (quant_fp8.hip, zero_amax).
__global__ __launch_bounds__(256) void amax_zero(unsigned* __restrict__ row, long rows, unsigned* __restrict__ col,
                                                 long cols, unsigned* __restrict__ ten) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows + cols + 1; i += stride) {
    if (i < rows) {
      if (row != nullptr) row[i] = 0u;
    } else if (i < rows + cols) {
      if (col != nullptr) col[i - rows] = 0u;
    } else if (ten != nullptr) {
      ten[0] = 0u;
    }
  }
}

// A tile is 128 rows x 256 columns; a workgroup takes the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... Thread (c, rq) = (t & 31, t >> 5) reads the 16-B
// chunk c of the rows 64 it + 8 rq + j (j < 8, it < 2): eight loads issued
// before the first use (hipcc hoists the second step's eight as well), each
// half-wave reading one contiguous 512-B row segment. |x| of a bf16 is its
// low 15 bits, and those order like the fp32 bit patterns they widen to, so
// the maxima are taken on 16-bit integers.
//   rows   : butterfly over the 32 lanes that share a row, then lane c < 8
//            issues row 8 rq + c (eight contiguous words per half-wave)
//   columns: kept in registers over the tile's 128 rows, merged through LDS,
//            256 contiguous atomics per tile
//   tensor : kept in registers over all of the workgroup's tiles, ONE atomic
//            per workgroup, and none when the word already holds as much:
//            atomics on one address run one after the other (a few ns each),
//            so when the tensor amax is asked for the grid is capped at
//            AM_MAX_WGS workgroups. Without it the grid is one workgroup per
//            tile (LOOP = false, fewer registers, four waves per SIMD): the row
//            and column atomics hide better behind more waves.
constexpr int AM_ROWS = 128, AM_COLS = 256, AM_MAX_WGS = 512;

template <bool LOOP>
__global__ __launch_bounds__(256) void amax_tile(const unsigned short* __restrict__ x, int rows, int cols, long ld,
                                                 unsigned* __restrict__ row_amax, unsigned* __restrict__ col_amax,
                                                 unsigned* __restrict__ ten_amax, int strips, int tiles) {
  __shared__ unsigned cred[4][32][8];
  __shared__ unsigned tred[4];
  const int t = threadIdx.x, c = t & 31, rq = t >> 5, lane = t & 63, wave = t >> 6;
  unsigned tm = 0u;
  int tile = blockIdx.x;  // < tiles: the grid is never larger
  do {
    const int br = tile / strips, bc = tile - br * strips;
    const long row0 = (long)AM_ROWS * br;
    const int col = AM_COLS * bc + 8 * c;
    const bool cin = col < cols;
    unsigned cm[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long rbase = row0 + 64 * it + 8 * rq;
      bf16x8 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (cin && rbase + j < rows) v[j] = *(const bf16x8*)(x + (rbase + j) * ld + col);
      }
      unsigned rm[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned m = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned a = (unsigned)(unsigned short)v[j][e] & 0x7fffu;
          cm[e] = max(cm[e], a);
          m = max(m, a);
        }
        rm[j] = m;
      }
      if (row_amax != nullptr) {
        unsigned mine = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unsigned m = rm[j];
#pragma unroll
          for (int o = 16; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
          mine = c == j ? m : mine;
        }
        if (c < 8 && rbase + c < rows) atomicMax(row_amax + rbase + c, mine << 16);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tm = max(tm, cm[e]);
    if (col_amax != nullptr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cm[e] = max(cm[e], (unsigned)__shfl_xor((int)cm[e], 32, 64));
      if (lane < 32) {
#pragma unroll
        for (int e = 0; e < 8; ++e) cred[wave][c][e] = cm[e];
      }
      __syncthreads();
      const int cc = AM_COLS * bc + t;
      const unsigned m = max(max(cred[0][t >> 3][t & 7], cred[1][t >> 3][t & 7]),
                             max(cred[2][t >> 3][t & 7], cred[3][t >> 3][t & 7]));
      if (cc < cols) atomicMax(col_amax + cc, m << 16);
      if constexpr (LOOP) __syncthreads();  // the next tile writes cred again
    }
  } while (LOOP && (tile += gridDim.x) < tiles);
  if (ten_amax != nullptr) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) tm = max(tm, (unsigned)__shfl_xor((int)tm, o, 64));
    if (lane == 0) tred[wave] = tm;
    __syncthreads();
    if (t == 0) {
      const unsigned m = max(max(tred[0], tred[1]), max(tred[2], tred[3])) << 16;
      // the word only grows: a value read now that is already >= m makes the atomic a no-op
      if (__hip_atomic_load(ten_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < m) atomicMax(ten_amax, m);
    }
  }
}

// ---------------------------------------------------------------------------
// A workgroup owns a 128 x 128 tile. Thread (c, q) = (t & 15, t >> 4) reads the
// 16-B chunk c (columns 8 c .. 8 c + 7) of the rows 64 g + 4 q + j (j < 4,
// g < 2): eight loads in flight, each 16-lane group reading 256 contiguous
// bytes of one row.
//
//   y : the thread's eight codes of a row are one 8-B store (128 contiguous
//       bytes per 16 lanes), straight from registers.
//   yt: v_cvt_pk_fp8_f32 packs the four rows j of ONE column into a dword, so
//       the 4 x 8 block a thread holds leaves it as eight dwords that are
//       already transposed. They go to the LDS tile
//
//         T[column 0..127][128 bytes = rows 0..127],   row pitch 128 B,
//         the 16-B slot s of column n stored at slot s ^ ((n >> 3) & 7)
//
//       and the tile is read back with ds_read_b128: thread (k, n) = (t & 7,
//       (t >> 3) + 32 p) takes slot k of column n -- rows 16 k .. 16 k + 15 --
//       and stores those 16 bytes to yt (128 contiguous bytes per 8 lanes).
//       Banks: a ds_read_b128 lane group holds halves of four consecutive
//       columns, e.g. lanes {0-3, 12-15, 20-27} = (n0, slots 0-3), (n0 + 1,
//       slots 4-7), (n0 + 2, slots 4-7), (n0 + 3, slots 0-3); a column's
//       parity picks the 128-B half of the 64 banks and the XOR, the same for
//       the eight columns of a wave pass, permutes the slots: 16 distinct
//       slots, no conflict. The XOR is there for the ds_write_b32: within a
//       32-lane group the dword index (q + 16 g) has only two values, and
//       without it the 16 chunks c would all meet on one bank; with it chunks
//       c and c + 8 share one, a two-way store conflict, which costs nothing
//       on ds_write_b32.
//
// The scale of a row / column / tensor is derived by every thread that needs
// it and written by exactly one workgroup: the row scales by the tiles of
// tile-column 0, the column scales by those of tile-row 0, a per-tensor scale
// by tile 0. No atomics.
constexpr int QT = 128;

template <bool HAS_Y, bool HAS_YT>
__global__ __launch_bounds__(256) void quant_tile(const unsigned short* __restrict__ x, int rows, int cols, long ld,
                                                  const float* __restrict__ row_amax,
                                                  const float* __restrict__ col_amax,
                                                  const float* __restrict__ ten_amax, unsigned char* __restrict__ y,
                                                  long ldy, float* __restrict__ y_scale,
                                                  unsigned char* __restrict__ yt, long ldyt,
                                                  float* __restrict__ yt_scale, const float* __restrict__ y_fold,
                                                  const float* __restrict__ yt_fold, int tiles_c) {
  __shared__ uint4 tile[QT * QT / 16];
  const int t = threadIdx.x, c = t & 15, q = t >> 4;
  const int tr = blockIdx.x / tiles_c, tc = blockIdx.x - tr * tiles_c;
  const long row0 = (long)QT * tr;
  const int col0 = QT * tc, col = col0 + 8 * c;
  const bool cin = col < cols;

  bf16x8 v[2][4];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long r = row0 + 64 * g + 4 * q + j;
      v[g][j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (cin && r < rows) v[g][j] = *(const bf16x8*)(x + r * ld + col);
    }
  }

  const float tscale = ten_amax != nullptr ? scale_of(ten_amax[0]) : 1.f;
  const float tinv = 1.f / tscale;

  if constexpr (HAS_Y) {
    const float fold = y_fold != nullptr ? y_fold[0] : 1.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long r = row0 + 64 * g + 4 * q + j;
        if (r < rows) {
          float inv = tinv;
          if (row_amax != nullptr) {
            const float sc = scale_of(row_amax[r]);
            inv = 1.f / sc;
            if (tc == 0 && c == 0 && y_scale != nullptr) y_scale[r] = sc * fold;
          }
          if (cin) {
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = clamp448(bf2f((unsigned short)v[g][j][e]) * inv);
            unsigned lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
            unsigned hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
            *(uint2*)(y + r * ldy + col) = make_uint2(lo, hi);
          }
        }
      }
    }
    if (row_amax == nullptr && blockIdx.x == 0 && t == 0 && y_scale != nullptr) y_scale[0] = tscale * fold;
  }

  if constexpr (HAS_YT) {
    const float fold = yt_fold != nullptr ? yt_fold[0] : 1.f;
    float cinv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      cinv[e] = tinv;
      if (col_amax != nullptr && cin) {
        const float sc = scale_of(col_amax[col + e]);
        cinv[e] = 1.f / sc;
        if (tr == 0 && q == 0 && yt_scale != nullptr) yt_scale[col + e] = sc * fold;
      }
    }
    if (col_amax == nullptr && blockIdx.x == 0 && t == 0 && yt_scale != nullptr) yt_scale[0] = tscale * fold;
    unsigned* tw = (unsigned*)tile;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int w = q + 16 * g;  // dword of the column's 128 bytes: rows 4 w .. 4 w + 3
      const int pos = (((w >> 2) ^ (c & 7)) << 2) | (w & 3);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f0 = clamp448(bf2f((unsigned short)v[g][0][e]) * cinv[e]);
        const float f1 = clamp448(bf2f((unsigned short)v[g][1][e]) * cinv[e]);
        const float f2 = clamp448(bf2f((unsigned short)v[g][2][e]) * cinv[e]);
        const float f3 = clamp448(bf2f((unsigned short)v[g][3][e]) * cinv[e]);
        unsigned d = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
        d = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, d, true);
        tw[(8 * c + e) * (QT / 4) + pos] = d;
      }
    }
    __syncthreads();
    const int k = t & 7;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int n = (t >> 3) + 32 * p;
      const uint4 o = tile[n * (QT / 16) + (k ^ ((n >> 3) & 7))];
      const long r = row0 + 16 * k;
      if (col0 + n < cols && r < rows) *(uint4*)(yt + (long)(col0 + n) * ldyt + r) = o;
    }
  }
}

}  // namespace f8t
}  // namespace kgs

static inline bool f8t_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline int f8t_shape(int rows, int cols, long ld) {
  if (rows <= 0 || cols <= 0 || rows % 16 || cols % 16 || ld < cols) return KGS_ERR_SHAPE;
  return 0;
}

// x: [rows, ld] bf16, rows % 16 == 0, cols % 16 == 0, ld % 8 == 0, 16-B aligned.
// row_amax [rows], col_amax [cols], tensor_amax [1]: fp32, each optional, at
// least one given; a null output is not touched. Two launches (reset, reduce),
// nothing allocated, nothing synchronised.
KGS_EXPORT int kgs_fp8_amax_bf16(const void* x, int rows, int cols, long ld, float* row_amax, float* col_amax,
                                 float* tensor_amax, hipStream_t s) {
  if (const int rc = f8t_shape(rows, cols, ld)) return rc;
  if (x == nullptr || (row_amax == nullptr && col_amax == nullptr && tensor_amax == nullptr)) return KGS_ERR_ARG;
  if (!f8t_al(x, 16) || ld % 8 || !f8t_al(row_amax, 4) || !f8t_al(col_amax, 4) || !f8t_al(tensor_amax, 4))
    return KGS_ERR_ALIGN;
  using namespace kgs::f8t;
  const long strips = ((long)cols + AM_COLS - 1) / AM_COLS, tiles = strips * (((long)rows + AM_ROWS - 1) / AM_ROWS);
  if (tiles > 0x7fffffffL) return KGS_ERR_SHAPE;
  const bool loop = tensor_amax != nullptr && tiles > AM_MAX_WGS;
  const dim3 g((unsigned)(loop ? AM_MAX_WGS : tiles)), b(256);
  const long nz = ((long)rows + cols + 1 + 255) / 256;
  hipLaunchKernelGGL(amax_zero, dim3((unsigned)(nz < 1024 ? nz : 1024)), dim3(256), 0, s, (unsigned*)row_amax,
                     (long)rows, (unsigned*)col_amax, (long)cols, (unsigned*)tensor_amax);
  if (loop)
    hipLaunchKernelGGL(amax_tile<true>, g, b, 0, s, (const unsigned short*)x, rows, cols, ld, (unsigned*)row_amax,
                       (unsigned*)col_amax, (unsigned*)tensor_amax, (int)strips, (int)tiles);
  else
    hipLaunchKernelGGL(amax_tile<false>, g, b, 0, s, (const unsigned short*)x, rows, cols, ld, (unsigned*)row_amax,
                       (unsigned*)col_amax, (unsigned*)tensor_amax, (int)strips, (int)tiles);
  return (int)hipGetLastError();
}

// x as above; the amax vectors are kgs_fp8_amax_bf16's outputs.
//   y  [rows, ldy]  e4m3, ldy % 16 == 0: scaled per row when row_amax is given
//      (y_scale: rows floats), else per tensor from tensor_amax (y_scale: 1).
//   yt [cols, ldyt] e4m3, ldyt % 16 == 0, the transpose: scaled per output row
//      when col_amax is given (yt_scale: cols floats), else per tensor (1).
// Either image may be null (not both); a null scale pointer skips that store.
// y_fold / yt_fold: optional device scalars multiplied into the stored scales
// only. With both images per tensor yt is y transposed bit for bit. One launch.
KGS_EXPORT int kgs_fp8_quant_bf16(const void* x, int rows, int cols, long ld, const float* row_amax,
                                  const float* col_amax, const float* tensor_amax, void* y, long ldy, float* y_scale,
                                  void* yt, long ldyt, float* yt_scale, const float* y_fold, const float* yt_fold,
                                  hipStream_t s) {
  if (const int rc = f8t_shape(rows, cols, ld)) return rc;
  if (x == nullptr || (y == nullptr && yt == nullptr)) return KGS_ERR_ARG;
  if (y != nullptr && ldy < cols) return KGS_ERR_SHAPE;
  if (yt != nullptr && ldyt < rows) return KGS_ERR_SHAPE;
  if (y != nullptr && row_amax == nullptr && tensor_amax == nullptr) return KGS_ERR_ARG;
  if (yt != nullptr && col_amax == nullptr && tensor_amax == nullptr) return KGS_ERR_ARG;
  if (!f8t_al(x, 16) || ld % 8 || !f8t_al(y, 16) || !f8t_al(yt, 16)) return KGS_ERR_ALIGN;
  if ((y != nullptr && ldy % 16) || (yt != nullptr && ldyt % 16)) return KGS_ERR_ALIGN;
  if (!f8t_al(row_amax, 4) || !f8t_al(col_amax, 4) || !f8t_al(tensor_amax, 4) || !f8t_al(y_scale, 4) ||
      !f8t_al(yt_scale, 4) || !f8t_al(y_fold, 4) || !f8t_al(yt_fold, 4))
    return KGS_ERR_ALIGN;
  using namespace kgs::f8t;
  const long tiles_c = ((long)cols + QT - 1) / QT, blocks = tiles_c * (((long)rows + QT - 1) / QT);
  if (blocks > 0x7fffffffL) return KGS_ERR_SHAPE;
  // an image scaled per row / column does not read the tensor amax, and the
  // other way round: hand the kernel only what the images it writes use
  const float* ra = y != nullptr ? row_amax : nullptr;
  const float* ca = yt != nullptr ? col_amax : nullptr;
  const float* ta = (y != nullptr && ra == nullptr) || (yt != nullptr && ca == nullptr) ? tensor_amax : nullptr;
  const dim3 g((unsigned)blocks), b(256);
#define KGS_Q(HY, HT)                                                                                              \
  hipLaunchKernelGGL((quant_tile<HY, HT>), g, b, 0, s, (const unsigned short*)x, rows, cols, ld, ra, ca, ta,       \
                     (unsigned char*)y, ldy, y_scale, (unsigned char*)yt, ldyt, yt_scale, y_fold, yt_fold,          \
                     (int)tiles_c)
  if (y != nullptr && yt != nullptr) KGS_Q(true, true);
  else if (y != nullptr) KGS_Q(true, false);
  else KGS_Q(false, true);
#undef KGS_Q
  return (int)hipGetLastError();
}
