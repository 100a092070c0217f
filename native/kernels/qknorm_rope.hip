// QK-norm fused with RoPE for gfx950: the per-head RMSNorm that Qwen3, OLMo-2 and
// Gemma-3 apply to q and k before the rotation, forward and backward, on the
// fused QKV row [tokens, (H + 2 HKV) * 128] the projection writes.
//
//   * qknorm_rope_fwd : per head row x (128 values) of the H q heads (w = wq) and
//                       the HKV k heads (w = wk), in place:
//                         r = rsqrt(mean(x^2) + eps),  n = (x r) w   (fp32, not rounded)
//                         out = bf16(rotate_half(n, cos[p], sin[p]))
//                       and, when asked, the pre-norm head rows to `save` in the
//                       same pass. The v heads are not touched.
//   * qknorm_rope_bwd : from dy (the whole fused row) and the saved pre-norm rows,
//                       out of place:
//                         g  = rotate_half(dy, cos[p], -sin[p]),  nh = x r,  gw = g w
//                         dx = bf16(r (gw - nh mean(gw nh))),     dv = dy's bits
//                       and one fp32 partial of dw = sum g nh per workgroup;
//   * qknorm_dw       : the partials summed per column in a fixed tree, rounded once.
//
// House rules (attention_train.hip): fp32 math, one bf16 rounding per output
// element, 16-B accesses, no float atomics, no workgroup waits on another.
//
// Work split. Eight lanes own one head row (256 B): lane c of the eight holds the
// 16-B chunk c of the first half and chunk c of the second half, rope_qkv's
// ownership, so every rotate-half pair (i, i + 64) lives in one lane and the
// rotation needs no cross-lane traffic. A wave covers eight head rows per trip,
// a workgroup 32. Both row sums (sum x^2, sum gw x) are 8-lane butterflies on DPP
// (two quad_perms and a row_half_mirror): no LDS and no barrier in the row loop.
// mean(gw nh) = r mean(gw x), so the backward's two butterflies do not depend on
// each other and issue together. A group of eight lanes enters or leaves the row
// loop as one, so a DPP step never reads a lane that is switched off.
//
// The q head rows, the k head rows and (backward) the v head rows are separate
// regions of a 1-D grid: a workgroup belongs to one region, so its lanes hold ONE
// weight in registers for the whole walk, and a lane's 16 fp32 dw accumulators
// only ever see that weight. Each region's workgroups walk its head rows with
// the region's grid stride. The grids are capped (FWD_WGS / BWD_WGS workgroups,
// split over the regions by the bytes a head row moves), so the weight, and in
// the backward the accumulators, are set up once per ~T H / 32 / cap trips.
//
// dwq / dwk. After the loop a lane's accumulators go to LDS; thread j < 128 adds
// column j's 32 values (wave 0 slot 0..7, wave 1 ..., in that order) and the
// workgroup stores one fp32 partial [128]. qknorm_dw sums the partials of a
// column in groups of consecutive partials, then the groups in order
// (rmsnorm_bwd_dw's tree). Grid, stride and tree follow from (tokens, H, HKV)
// alone: bitwise repeatable, capturable in a hipGraph.
//
// One departure from rope_qkv: the entries take the tables' row count and the
// kernels clamp a position into it, so a bad `pos` entry reads a wrong table row
// instead of memory outside the tables.
#include "kgs_common.h"

namespace kgs {
namespace qkn {

constexpr int HD = 128;        // the only head dim
constexpr int WG_ROWS = 32;    // head rows per workgroup trip: 4 waves x 8 slots
constexpr int FWD_WGS = 2048;  // default grid caps, measured (profiles/r17/qknorm_rope/README.md)
constexpr int BWD_WGS = 1024;
constexpr int MAX_WGS = 8192;  // the workspace is sized for this many partials

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// The sum over the 8 lanes of a head row, the same bits in all 8: lane ^ 1, lane
// ^ 2 (quad_perm [1,0,3,2], [2,3,0,1]), then the other quad of the eight through
// row_half_mirror (lane 7 - i: every lane of a quad already holds the quad's sum).
__device__ __forceinline__ float sum8(float v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x141>(v);
  return v;
}

__device__ __forceinline__ void unpack(float (&f)[16], const bf16x8 lo, const bf16x8 hi) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = bf2f((unsigned short)lo[e]);
    f[8 + e] = bf2f((unsigned short)hi[e]);
  }
}

// cos / sin of table row p for this lane's 8 pairs
__device__ __forceinline__ void table8(float (&o)[8], const float* __restrict__ tab, int p, int c) {
  const f32x4* tp = (const f32x4*)(tab + (long)p * (HD / 2) + 8 * c);
  const f32x4 a = tp[0], b = tp[1];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = a[e];
    o[4 + e] = b[e];
  }
}

__device__ __forceinline__ int position(const int* __restrict__ pos, unsigned t, int seq, int npos) {
  const int p = pos != nullptr ? pos[t] : (int)(t % (unsigned)seq);
  return min(max(p, 0), npos - 1);
}

__global__ __launch_bounds__(256) void qknorm_rope_fwd(unsigned short* qkv, unsigned short* __restrict__ save,
                                                       const unsigned short* __restrict__ wq,
                                                       const unsigned short* __restrict__ wk,
                                                       const float* __restrict__ cosv, const float* __restrict__ sinv,
                                                       const int* __restrict__ pos, int heads, int kv_heads,
                                                       unsigned rows_q, unsigned rows_k, unsigned wgs_q,
                                                       unsigned wgs_k, long ld, long ldsave, int seq, int npos,
                                                       float eps) {
  const bool isk = blockIdx.x >= wgs_q;  // workgroup-uniform: the k region follows the q region
  const unsigned nh = isk ? kv_heads : heads, h0 = isk ? heads : 0;
  const unsigned rows = isk ? rows_k : rows_q;
  const unsigned stride = (isk ? wgs_k : wgs_q) * WG_ROWS;
  const int c = threadIdx.x & 7;
  const bf16x8* wp = (const bf16x8*)(isk ? wk : wq);
  float w[16];
  unpack(w, wp[c], wp[8 + c]);

  for (unsigned row = (isk ? blockIdx.x - wgs_q : blockIdx.x) * WG_ROWS + (threadIdx.x >> 3); row < rows;
       row += stride) {
    const unsigned t = row / nh;
    const long col = (long)(h0 + (row - t * nh)) * HD + 8 * c;
    bf16x8* p1 = (bf16x8*)(qkv + t * ld + col);
    const bf16x8 a = p1[0], b = p1[HD / 16];
    const int p = position(pos, t, seq, npos);
    float cs[8], sn[8], x[16];
    table8(cs, cosv, p, c);
    table8(sn, sinv, p, c);
    if (save != nullptr) {
      bf16x8* sp = (bf16x8*)(save + t * ldsave + col);
      __builtin_nontemporal_store(a, sp);
      __builtin_nontemporal_store(b, sp + HD / 16);
    }
    unpack(x, a, b);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) ss += x[e] * x[e];
    const float r = rsqrtf(sum8(ss) * (1.f / HD) + eps);
    float lo[8], hi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float n1 = (x[e] * r) * w[e], n2 = (x[8 + e] * r) * w[8 + e];
      lo[e] = rope_lo(n1, n2, cs[e], sn[e]);
      hi[e] = rope_hi(n1, n2, cs[e], sn[e]);
    }
    p1[0] = pack_bf16x8(lo, 0);
    p1[HD / 16] = pack_bf16x8(hi, 0);
  }
}

__global__ __launch_bounds__(256) void qknorm_rope_bwd(const unsigned short* __restrict__ dy,
                                                       const unsigned short* __restrict__ save,
                                                       const unsigned short* __restrict__ wq,
                                                       const unsigned short* __restrict__ wk,
                                                       const float* __restrict__ cosv, const float* __restrict__ sinv,
                                                       const int* __restrict__ pos, unsigned short* __restrict__ dx,
                                                       float* __restrict__ ws, int heads, int kv_heads,
                                                       unsigned rows_q, unsigned rows_k, unsigned wgs_q,
                                                       unsigned wgs_k, unsigned wgs_v, long lddy, long ldsave,
                                                       long lddx, int seq, int npos, float eps) {
  const int c = threadIdx.x & 7;
  const unsigned slot = threadIdx.x >> 3;
  if (blockIdx.x >= wgs_q + wgs_k) {  // workgroup-uniform: the v region, a copy of dy's v head rows
    const unsigned stride = wgs_v * WG_ROWS;
    for (unsigned row = (blockIdx.x - wgs_q - wgs_k) * WG_ROWS + slot; row < rows_k; row += stride) {
      const unsigned t = row / (unsigned)kv_heads;
      const long col = (long)(heads + kv_heads + (row - t * kv_heads)) * HD + 8 * c;
      const bf16x8* src = (const bf16x8*)(dy + t * lddy + col);
      const bf16x8 a = __builtin_nontemporal_load(src), b = __builtin_nontemporal_load(src + HD / 16);
      bf16x8* dst = (bf16x8*)(dx + t * lddx + col);
      dst[0] = a;
      dst[HD / 16] = b;
    }
    return;
  }
  const bool isk = blockIdx.x >= wgs_q;
  const unsigned nh = isk ? kv_heads : heads, h0 = isk ? heads : 0;
  const unsigned rows = isk ? rows_k : rows_q;
  const unsigned stride = (isk ? wgs_k : wgs_q) * WG_ROWS;
  const bf16x8* wp = (const bf16x8*)(isk ? wk : wq);
  float w[16], acc[16];
  unpack(w, wp[c], wp[8 + c]);
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  for (unsigned row = (isk ? blockIdx.x - wgs_q : blockIdx.x) * WG_ROWS + slot; row < rows; row += stride) {
    const unsigned t = row / nh;
    const long col = (long)(h0 + (row - t * nh)) * HD + 8 * c;
    const bf16x8* gp = (const bf16x8*)(dy + t * lddy + col);
    const bf16x8* xp = (const bf16x8*)(save + t * ldsave + col);
    const bf16x8 ga = __builtin_nontemporal_load(gp), gb = __builtin_nontemporal_load(gp + HD / 16);
    const bf16x8 xa = __builtin_nontemporal_load(xp), xb = __builtin_nontemporal_load(xp + HD / 16);
    const int p = position(pos, t, seq, npos);
    float cs[8], sn[8], x[16], d[16], g[16];
    table8(cs, cosv, p, c);
    table8(sn, sinv, p, c);
    unpack(x, xa, xb);
    unpack(d, ga, gb);
    float ss = 0.f, gx = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // the transposed rotation: rope_qkv's backward, the rotation by -angle
      g[e] = rope_lo(d[e], d[8 + e], cs[e], -sn[e]);
      g[8 + e] = rope_hi(d[e], d[8 + e], cs[e], -sn[e]);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      ss += x[e] * x[e];
      gx += (g[e] * w[e]) * x[e];
    }
    ss = sum8(ss);
    gx = sum8(gx);
    const float r = rsqrtf(ss * (1.f / HD) + eps);
    const float m = r * (gx * (1.f / HD));  // mean(gw nh)
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float nhat = x[e] * r;
      o[e] = r * (g[e] * w[e] - nhat * m);
      acc[e] += g[e] * nhat;
    }
    bf16x8* op = (bf16x8*)(dx + t * lddx + col);
    op[0] = pack_bf16x8(o, 0);
    op[HD / 16] = pack_bf16x8(o, 8);
  }

  // the workgroup's partial: wave 0 slot 0 .. 7, wave 1 slot 0 .. 7, ... in that order
  __shared__ float red[WG_ROWS][HD];
  f32x4* mine = (f32x4*)&red[slot][8 * c];
  mine[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  mine[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  mine[HD / 8] = f32x4{acc[8], acc[9], acc[10], acc[11]};
  mine[HD / 8 + 1] = f32x4{acc[12], acc[13], acc[14], acc[15]};
  __syncthreads();
  if (threadIdx.x < HD) {
    float s = red[0][threadIdx.x];
#pragma unroll 8
    for (int q = 1; q < WG_ROWS; ++q) s += red[q][threadIdx.x];
    ws[(long)blockIdx.x * HD + threadIdx.x] = s;
  }
}

// dwq / dwk = bf16(sum of the partials). Workgroup b: weight b >> 1 (q, k), column
// half b & 1. Thread (oct, grp) = (t & 7, t >> 3) sums the partials grp * per ..
// (grp + 1) * per - 1 of column octet oct in index order, then the 32 group sums
// are added in group order through LDS (rmsnorm_bwd_dw's tree).
__global__ __launch_bounds__(256) void qknorm_dw(const float* __restrict__ ws, unsigned short* __restrict__ dwq,
                                                 unsigned short* __restrict__ dwk, int parts_q, int parts_k) {
  __shared__ f32x4 red[32][2][8];
  const bool isk = blockIdx.x >> 1;
  const float* base = ws + (isk ? (long)parts_q * HD : 0);
  const int nparts = isk ? parts_k : parts_q;
  const int oct = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int c8 = 8 * (blockIdx.x & 1) + oct;  // this thread's column octet of the 16
  const int per = (nparts + 31) / 32;
  const int p1 = min(nparts, (grp + 1) * per);
  f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
  for (int p = grp * per; p < p1; ++p) {
    const f32x4* pr = (const f32x4*)(base + (long)p * HD) + 2 * c8;
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
    ((bf16x8*)(isk ? dwk : dwq))[c8] = pack_bf16x8(o, 0);
  }
}

// The regions' workgroup counts: the cap split by the bytes a head row of each
// region moves (3 x 256 B for q and k, 2 x 256 B for the backward's v copy), at
// least one each, and never more than the region has 32-row trips.
struct Grid {
  unsigned rows_q, rows_k, q, k, v;
};

static inline unsigned region_wgs(long cap, long share, long total, unsigned rows) {
  const long want = cap * share / total, trips = ((long)rows + WG_ROWS - 1) / WG_ROWS;
  return (unsigned)(want < 1 ? 1 : (want < trips ? want : trips));
}

static inline Grid grid_for(long tokens, int heads, int kv_heads, int cap, bool with_v) {
  Grid g;
  g.rows_q = (unsigned)(tokens * heads);
  g.rows_k = (unsigned)(tokens * kv_heads);
  const long total = 3L * heads + 3L * kv_heads + (with_v ? 2L * kv_heads : 0);
  g.q = region_wgs(cap, 3L * heads, total, g.rows_q);
  g.k = region_wgs(cap, 3L * kv_heads, total, g.rows_k);
  g.v = with_v ? region_wgs(cap, 2L * kv_heads, total, g.rows_k) : 0;
  return g;
}

}  // namespace qkn
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline int qkn_shape(long tokens, int heads, int kv_heads, int hd, int wgs) {
  if (tokens < 0 || heads < 1 || kv_heads < 1 || hd != kgs::qkn::HD) return KGS_ERR_SHAPE;
  if (wgs < 0 || wgs > kgs::qkn::MAX_WGS) return KGS_ERR_SHAPE;
  const long most = heads > kv_heads ? heads : kv_heads;
  if (tokens > 0x7fffffffL / most) return KGS_ERR_SHAPE;  // head-row indices are 32-bit
  return 0;
}

// Bytes of the fp32 workspace kgs_qknorm_rope_bwd_bf16 needs (one partial [128]
// per workgroup of the q and k regions, whatever grid cap is asked for), or
// KGS_ERR_SHAPE. At least 16, so there is always a buffer.
KGS_EXPORT long kgs_qknorm_rope_bwd_workspace(long tokens, int heads, int kv_heads) {
  using namespace kgs::qkn;
  if (qkn_shape(tokens, heads, kv_heads, HD, 0)) return KGS_ERR_SHAPE;
  const Grid g = grid_for(tokens, heads, kv_heads, MAX_WGS, true);
  const long b = tokens == 0 ? 0 : ((long)g.q + g.k) * HD * 4;
  return b < 16 ? 16 : b;
}

// qkv: bf16 [tokens, ld], the H q heads, the HKV k heads, then the v heads, 128
// wide each; normalised and rotated in place, the v heads untouched. save:
// optional bf16 [tokens, ldsave], receives the pre-norm q and k heads (its first
// (H + HKV) * 128 columns). wq, wk: bf16 [128]. cos / sin: fp32 [npos, 64]. pos:
// optional int32 [tokens], else position = token % seq (then seq <= npos). wgs:
// the grid cap, 0 for the default. tokens == 0 launches nothing.
KGS_EXPORT int kgs_qknorm_rope_fwd_bf16(void* qkv, void* save, const void* wq, const void* wk, const float* cosv,
                                       const float* sinv, const int* pos, long tokens, int heads, int kv_heads,
                                       int hd, long ld, long ldsave, int seq, int npos, float eps, int wgs,
                                       hipStream_t s) {
  using namespace kgs::qkn;
  if (const int rc = qkn_shape(tokens, heads, kv_heads, hd, wgs)) return rc;
  if (ld < (long)(heads + 2 * kv_heads) * HD || (save && ldsave < (long)(heads + kv_heads) * HD) || npos < 1)
    return KGS_ERR_SHAPE;
  if (!pos && (seq < 1 || seq > npos)) return KGS_ERR_ARG;
  if (!qkv || !wq || !wk || !cosv || !sinv) return KGS_ERR_ALIGN;
  if (!al16(qkv) || !al16(save) || !al16(wq) || !al16(wk) || !al16(cosv) || !al16(sinv) || ((uintptr_t)pos & 3))
    return KGS_ERR_ALIGN;
  if (ld % 8 || (save && ldsave % 8)) return KGS_ERR_ALIGN;
  if (tokens == 0) return 0;
  const Grid g = grid_for(tokens, heads, kv_heads, wgs ? wgs : FWD_WGS, false);
  hipLaunchKernelGGL(qknorm_rope_fwd, dim3(g.q + g.k), dim3(256), 0, s, (unsigned short*)qkv, (unsigned short*)save,
                     (const unsigned short*)wq, (const unsigned short*)wk, cosv, sinv, pos, heads, kv_heads, g.rows_q,
                     g.rows_k, g.q, g.k, ld, ldsave, seq, npos, eps);
  return (int)hipGetLastError();
}

// dy: bf16 [tokens, lddy], the gradient of the whole fused row, only read. save:
// bf16 [tokens, ldsave], the forward's pre-norm q and k heads. dx: bf16 [tokens,
// lddx], every one of its (H + 2 HKV) * 128 columns written (the v columns are
// dy's bits); dx must not overlap dy. dwq, dwk: bf16 [128]. ws: fp32 workspace of
// kgs_qknorm_rope_bwd_workspace(tokens, heads, kv_heads) bytes. Two launches,
// nothing allocated, nothing synchronised. tokens == 0 launches nothing and
// writes nothing.
KGS_EXPORT int kgs_qknorm_rope_bwd_bf16(const void* dy, const void* save, const void* wq, const void* wk,
                                       const float* cosv, const float* sinv, const int* pos, void* dx, void* dwq,
                                       void* dwk, void* ws, long tokens, int heads, int kv_heads, int hd, long lddy,
                                       long ldsave, long lddx, int seq, int npos, float eps, int wgs, hipStream_t s) {
  using namespace kgs::qkn;
  if (const int rc = qkn_shape(tokens, heads, kv_heads, hd, wgs)) return rc;
  const long width = (long)(heads + 2 * kv_heads) * HD;
  if (lddy < width || lddx < width || ldsave < (long)(heads + kv_heads) * HD || npos < 1) return KGS_ERR_SHAPE;
  if (!pos && (seq < 1 || seq > npos)) return KGS_ERR_ARG;
  if (!dy || !save || !wq || !wk || !cosv || !sinv || !dx || !dwq || !dwk || !ws) return KGS_ERR_ALIGN;
  if (!al16(dy) || !al16(save) || !al16(wq) || !al16(wk) || !al16(cosv) || !al16(sinv) || !al16(dx) || !al16(dwq) ||
      !al16(dwk) || !al16(ws) || ((uintptr_t)pos & 3))
    return KGS_ERR_ALIGN;
  if (lddy % 8 || ldsave % 8 || lddx % 8) return KGS_ERR_ALIGN;
  if (tokens == 0) return 0;
  const Grid g = grid_for(tokens, heads, kv_heads, wgs ? wgs : BWD_WGS, true);
  hipLaunchKernelGGL(qknorm_rope_bwd, dim3(g.q + g.k + g.v), dim3(256), 0, s, (const unsigned short*)dy,
                     (const unsigned short*)save, (const unsigned short*)wq, (const unsigned short*)wk, cosv, sinv,
                     pos, (unsigned short*)dx, (float*)ws, heads, kv_heads, g.rows_q, g.rows_k, g.q, g.k, g.v, lddy,
                     ldsave, lddx, seq, npos, eps);
  hipLaunchKernelGGL(qknorm_dw, dim3(4), dim3(256), 0, s, (const float*)ws, (unsigned short*)dwq,
                     (unsigned short*)dwk, (int)g.q, (int)g.k);
  return (int)hipGetLastError();
}
