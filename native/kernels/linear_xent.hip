// Fused LM head + softmax cross-entropy (round 23): the logits z = h . w^T never reach memory.
//
// h: bf16 [T, K] (row stride ldh), w: bf16 [V, K] (row stride ldw), target: int64 [T]. A row whose
// target is outside [0, V) is ignored, as in xent_fwd (train_ops.hip).
//
//   fwd      lse[row] = log sum_j e^z[row, j] and loss[row] = lse - z[row, target] (0 for an
//            ignored row, whose lse is still written). Kept for the backward: lse alone.
//   dlogits  recomputes the tiles of the column range [v0, v0 + Vc) and stores
//            bf16(grow[row] . (e^(z - lse) - [col == target])) into a [T, Vc] buffer of its own;
//            ignored rows are zeros. At the target p - 1 is grow . expm1(z - lse): xent_bwd's sum of
//            the other columns is not available inside a tile, and expm1 adds no cancellation of its
//            own to the error z - lse already has. Where p is 1 in fp32, lse equals z bit for bit
//            and the entry is 0: short of the truth by grow . (1 - p) < grow . 2^-24.
//
// The logits are never rounded to bf16: both epilogues run on the fp32 accumulators. target is only
// ever compared with a column number, never used as an address. Every output element is written on
// every call (no memset in a captured step), there are no atomics, no workgroup waits on another,
// and the grid and the order of additions depend on the shapes only: results are bitwise repeatable.
//
// Design. The K loop is moe_gemm.hip's: tile BM x 128, BM / 64 x 2 waves of 64 x 64 each, 16
// accumulators of v_mfma_f32_16x16x32_bf16 per wave in ascending k, BK = 64, operands HBM -> LDS by
// LDS-DMA in the lane-linear XOR-swizzled image, NS stages, one barrier per K-step; 256 x 128 x 3
// stages where T % 256 == 0, else 128 x 128 x 2 stages.
// fwd: a workgroup owns one row tile and a strip of STRIP consecutive vocabulary tiles and walks
// them with a running (max m, sum of e^(z - m)) per row in registers. A lane holds 16 values of each
// of its 4 rows; per tile it takes their maximum, the 4 lanes that share a row merge the maximum by
// two half-swaps (so they agree on m), and each lane rescales and extends its OWN partial sum. The
// partial sums of the 4 lanes are added once, at the end of the strip, then the two column waves
// merge through LDS, once per strip, and one float2 (m, s) per row goes to the workspace
// [T, nstrips]. The one lane in the grid that holds (row, target[row]) stores that fp32 logit into
// tlogit[row]. A second kernel merges a row's partials in strip order.
// Grid: 1-D, xcd_remap gives every XCD a contiguous range of logical ids; ids go in groups of
// GROUP_M = 8 tile-rows, strip after strip inside a group, so the 32 workgroups an XCD runs at once
// are 8 row tiles x 4 strips: a w tile is fetched into that L2 once for 8 row tiles, an h tile
// once for 4 strips, the traffic of the plain GEMM. dlogits: the same order with one tile per
// workgroup; the store pairs n-tiles by v_permlane16_swap so that every lane writes 16 bytes.
#include "kgs_common.h"

namespace kgs {
namespace linear_xent {

constexpr int BN = 128, BK = 64, ROW = BK * 2, GROUP_M = 8, STRIP = 8;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr float FLOOR = -3.0e38f;  // a finite "-inf", as XENT_FLOOR: no inf - inf

struct Args {
  const unsigned short* H;
  const unsigned short* W;
  const long long* target;
  float2* part;           // fwd: [T, nstrips] (m, s)
  float* tlogit;          // fwd: [T]
  const float* lse;       // dlogits
  const float* grow;      // dlogits
  unsigned short* D;      // dlogits: [T, V] of this call's column range
  long ldh, ldw, ldd;
  int T, V, K;            // V: the columns this launch covers (W's rows)
  int nstrips;            // fwd: ceil(V / 128 / STRIP)
  int v0, vocab;          // dlogits: the range's first column, the whole vocabulary
};

__device__ __forceinline__ void bar() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// e^x on the bare v_exp_f32: exp2f's scaling for results below 2^-126 costs a compare and two
// multiplies per element of the tile, and such a term is nothing next to the row's maximum
__device__ __forceinline__ float ex(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }

template <int WM, int NS, bool BWD>
__global__ __launch_bounds__(WM * 128) void head_tiles(const Args p) {
  constexpr int BM = WM * 64, NW = WM * 2;
  constexpr int A_BYTES = BM * ROW, STAGE = (BM + BN) * ROW;
  constexpr int RB = BN / NW;        // w rows a wave loads per K-tile
  constexpr int GA = 4, GB = RB / 8; // 1-KiB DMAs per wave per K-tile: 32 h rows, RB w rows
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];
  __shared__ float2 red[BWD ? 1 : BM];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int ntm = p.T / BM, ntn = p.V / BN, ncol = BWD ? ntn : p.nstrips;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int group = id / (GROUP_M * ncol), first = group * GROUP_M, in_group = id - group * GROUP_M * ncol;
  const int gsz = min(ntm - first, GROUP_M);
  const int tm = first + in_group % gsz, sp = in_group / gsz;
  const int tn0 = BWD ? sp : sp * STRIP, tn1 = BWD ? sp + 1 : min(ntn, tn0 + STRIP);
  const int nt = p.K / BK;

  // DMA j of wave w fills rows w * 32 + j * 8 + lane / 8 of the h tile (w * RB + .. of the w
  // tile); the lane's physical chunk lane & 7 holds logical chunk (lane & 7) ^ ((row >> 1) & 7)
  const unsigned short* pa[GA];
  const unsigned short* pb[GB];
  {
    const unsigned short* At = p.H + (long)tm * BM * p.ldh;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const int r = w * 32 + j * 8 + (lane >> 3);
      pa[j] = At + r * p.ldh + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int r = w * RB + j * 8 + (lane >> 3);
      pb[j] = p.W + r * p.ldw + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
  }
  auto issue = [&](int stage, int k0, long wofs) {
    char* dst = smem + stage * STAGE;
#pragma unroll
    for (int j = 0; j < GA; ++j) glds16(pa[j] + k0, dst + w * 4096 + j * 1024);
#pragma unroll
    for (int j = 0; j < GB; ++j) glds16(pb[j] + wofs + k0, dst + A_BYTES + w * (RB * ROW) + j * 1024);
  };

  // fragment reads: row lane & 15 of a 16-row block, logical chunk 4 s + lane / 16
  const int fr = lane & 15, fq = lane >> 4;
  const int ro0 = fr * ROW + ((fq ^ (fr >> 1)) * 16), ro1 = fr * ROW + (((4 + fq) ^ (fr >> 1)) * 16);
  const int offa = wr * 64 * ROW, offb = A_BYTES + wc * 64 * ROW;

  // the lane's 4 rows: wr * 64 + i * 16 + fr. tg: the target as a column, far below 0 when ignored
  int tg[4];
  float m[4], s[4];  // fwd: running maximum (shared by the row's 4 lanes), the lane's own partial sum
  float lrow[4], grow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = (long)tm * BM + wr * 64 + i * 16 + fr;
    const long long t = p.target[row];
    tg[i] = (t >= 0 && t < (BWD ? p.vocab : p.V)) ? (int)t : -0x40000000;
    m[i] = FLOOR;
    s[i] = 0.f;
    lrow[i] = BWD ? p.lse[row] : 0.f;
    grow[i] = BWD ? p.grow[row] : 0.f;
  }

  for (int tn = tn0; tn < tn1; ++tn) {
    // every wave has read the last K-tile of the tile before (it waited for its fragments before
    // its MFMAs): after this barrier the stages may be filled again
    if (tn != tn0) bar();
    const long wofs = (long)tn * BN * p.ldw;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int j = 0; j < NS - 1; ++j)
      if (j < nt) issue(j, j * BK, wofs);

    int rs = 0, ws = NS - 1;  // the stage tile kt is read from, the stage tile kt + NS - 1 goes to
    for (int kt = 0; kt < nt; ++kt) {
      // tile kt has landed: at most the one tile issued after it may still be in flight
      if (NS > 2 && kt + 1 < nt) wait_vm<(NS > 2 ? GA + GB : 0)>(); else wait_vm<0>();
      bar();
      const char* st = smem + rs * STAGE;
      bf16x8 a[4][2], b[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i][0] = *(const bf16x8*)(st + offa + i * 16 * ROW + ro0);
        a[i][1] = *(const bf16x8*)(st + offa + i * 16 * ROW + ro1);
        b[i][0] = *(const bf16x8*)(st + offb + i * 16 * ROW + ro0);
        b[i][1] = *(const bf16x8*)(st + offb + i * 16 * ROW + ro1);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kt + NS - 1 < nt) issue(ws, (kt + NS - 1) * BK, wofs);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            // w first: the lane ends up with 4 consecutive columns of one row,
            // z[i * 16 + (lane & 15)][n * 16 + 4 * (lane >> 4) + 0 .. 3]
            acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n][ks], a[i][ks], acc[i][n], 0, 0, 0);
      rs = rs + 1 == NS ? 0 : rs + 1;
      ws = ws + 1 == NS ? 0 : ws + 1;
    }

    const int cb = tn * BN + wc * 64 + 4 * fq;  // the lane's column 0 of n-tile 0, inside this launch's range
    if constexpr (!BWD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float tmx = acc[i][0][0];
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) tmx = fmaxf(tmx, acc[i][n][j]);
        tmx = xor32_max(xor16_max(tmx));
        const float mn = fmaxf(m[i], tmx);
        float bs = 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) bs += ex(acc[i][n][j] - mn);
        s[i] = s[i] * ex(m[i] - mn) + bs;
        m[i] = mn;
        const int d = tg[i] - cb;  // = n * 16 + j when this lane holds the target
        if ((unsigned)d < 64u && (d & 12) == 0) {
          float v = 0.f;
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) v = d == n * 16 + j ? acc[i][n][j] : v;
          p.tlogit[(long)tm * BM + wr * 64 + i * 16 + fr] = v;
        }
      }
    } else {
      // store: v_permlane16_swap pairs the n-tiles so that every lane writes 16 bytes
      unsigned short* Dt = p.D + (long)tm * BM * p.ldd + tn * BN;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr * 64 + i * 16 + fr;
        unsigned short* drow = Dt + (long)row * p.ldd + wc * 64;
        const bool keep = tg[i] >= 0;
        const float l = lrow[i], g = grow[i];
        const int d = tg[i] - p.v0 - cb;
        f32x4 e[4];
        // + 0: a zero product keeps a positive sign (grow = 0: zero bits), as xent_bwd
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) e[n][j] = g * ex(acc[i][n][j] - l) + 0.0f;
        if ((unsigned)d < 64u && (d & 12) == 0) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) e[n][j] = d == n * 16 + j ? g * expm1f(acc[i][n][j] - l) + 0.0f : e[n][j];
        }
#pragma unroll
        for (int np = 0; np < 2; ++np) {
          const f32x4 v0 = e[2 * np], v1 = e[2 * np + 1];
          const unsigned x0 = pack_bf16x2(v0[0], v0[1]), y0 = pack_bf16x2(v0[2], v0[3]);
          const unsigned x1 = pack_bf16x2(v1[0], v1[1]), y1 = pack_bf16x2(v1[2], v1[3]);
          const auto sx = __builtin_amdgcn_permlane16_swap(x0, x1, false, false);
          const auto sy = __builtin_amdgcn_permlane16_swap(y0, y1, false, false);
          // even fq: 8 consecutive columns of n-tile 2 np; odd fq: of n-tile 2 np + 1
          const uint4 q = keep ? make_uint4(sx[0], sy[0], sx[1], sy[1]) : make_uint4(0, 0, 0, 0);
          *(uint4*)(drow + np * 32 + (fq & 1) * 16 + (fq >> 1) * 8) = q;
        }
      }
    }
  }

  if constexpr (!BWD) {
    // the row's 4 lanes hold the same m: add their sums (the same bits in all 4), then the
    // column wave 1 hands its pair to wave 0 of the same rows
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = xor32_sum(xor16_sum(s[i]));
    if (wc == 1 && fq == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wr * 64 + i * 16 + fr] = make_float2(m[i], s[i]);
    }
    __syncthreads();
    if (wc == 0 && fq == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr * 64 + i * 16 + fr;
        const float2 o = red[row];
        const float mn = fmaxf(m[i], o.x);
        const float sum = s[i] * ex(m[i] - mn) + o.y * ex(o.x - mn);
        p.part[((long)tm * BM + row) * p.nstrips + sp] = make_float2(mn, sum);
      }
    }
  }
}

// one thread per row: the strips' (m, s) merged in strip order
__global__ __launch_bounds__(256) void finish(const float2* __restrict__ part, const float* __restrict__ tlogit,
                                              const long long* __restrict__ target, float* __restrict__ loss,
                                              float* __restrict__ lse, int T, int V, int nstrips) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= T) return;
  const float2* pr = part + (long)row * nstrips;
  float m = pr[0].x, s = pr[0].y;
  for (int q = 1; q < nstrips; ++q) {
    const float2 o = pr[q];
    const float mn = fmaxf(m, o.x);
    s = s * ex(m - mn) + o.y * ex(o.x - mn);
    m = mn;
  }
  const float l = m + __log2f(s) * LN2;
  const long long tg = target[row];
  lse[row] = l;
  if (tg >= 0 && tg < V) loss[row] = l - tlogit[row]; else loss[row] = 0.f;
}

template <int WM, int NS, bool BWD>
static int launch(const Args& a, hipStream_t s) {
  const long grid = (long)(a.T / (WM * 64)) * (BWD ? a.V / BN : a.nstrips);
  if (a.T % (WM * 64) || grid > 0x7fffffffL) return KGS_ERR_SHAPE;
  hipLaunchKernelGGL((head_tiles<WM, NS, BWD>), dim3((unsigned)grid), dim3(WM * 128), 0, s, a);
  return (int)hipGetLastError();
}

static int check(const void* h, const void* w, const void* target, int T, int V, int K, long ldh, long ldw) {
  if (T < 128 || V < 128 || K < 64 || T % 128 || V % 128 || K % 64 || ldh < K || ldw < K) return KGS_ERR_SHAPE;
  if (!h || !w || !target || ((uintptr_t)h | (uintptr_t)w) % 16 || (uintptr_t)target % 8 || (ldh | ldw) % 8)
    return KGS_ERR_ALIGN;
  return 0;
}

static int strips(int V) { return (V / BN + STRIP - 1) / STRIP; }

}  // namespace linear_xent
}  // namespace kgs

// Bytes of the workspace kgs_linear_xent_fwd_bf16 needs: one float2 per row and strip, then one
// float per row for the target logit.
KGS_EXPORT long kgs_linear_xent_workspace(int T, int V) {
  using namespace kgs::linear_xent;
  if (T < 128 || V < 128 || T % 128 || V % 128) return KGS_ERR_SHAPE;
  return (long)T * strips(V) * 8 + (long)T * 4;
}

// loss, lse: fp32 [T]. ws: kgs_linear_xent_workspace(T, V) bytes. tile as in kgs_moe_gemm_bf16_nt:
// -1 in production = 256 x 128 x 3 stages where T % 256 == 0, else 128 x 128 x 2; 0 / 1 force one.
// Two launches, nothing allocated, nothing synchronised.
KGS_EXPORT int kgs_linear_xent_fwd_bf16(const void* h, const void* w, const void* target, float* loss, float* lse,
                                        void* ws, int T, int V, int K, long ldh, long ldw, int tile, hipStream_t s) {
  using namespace kgs::linear_xent;
  if (const int rc = check(h, w, target, T, V, K, ldh, ldw)) return rc;
  if (tile < -1 || tile > 1 || (tile == 1 && T % 256)) return KGS_ERR_ARG;
  if (!loss || !lse || !ws || (uintptr_t)ws % 16 || ((uintptr_t)loss | (uintptr_t)lse) % 4) return KGS_ERR_ALIGN;
  Args a = {};
  a.H = (const unsigned short*)h, a.W = (const unsigned short*)w, a.target = (const long long*)target;
  a.ldh = ldh, a.ldw = ldw, a.T = T, a.V = V, a.K = K;
  a.nstrips = strips(V);
  a.part = (float2*)ws, a.tlogit = (float*)((char*)ws + (long)T * a.nstrips * 8);
  if (tile < 0) tile = T % 256 == 0;
  if (const int rc = tile ? launch<4, 3, false>(a, s) : launch<2, 2, false>(a, s)) return rc;
  hipLaunchKernelGGL(finish, dim3((T + 255) / 256), dim3(256), 0, s, a.part, a.tlogit, a.target, loss, lse, T, V,
                     a.nstrips);
  return (int)hipGetLastError();
}

// dlogits of the columns [v0, v0 + Vc) of a vocabulary of vocab columns: w points at row v0 of the
// head's weight, out is bf16 [T, Vc] with row stride ldo, lse and grow are fp32 [T].
KGS_EXPORT int kgs_linear_xent_dlogits_bf16(const void* h, const void* w, const void* target, const float* lse,
                                            const float* grow, void* out, int T, int Vc, int K, long ldh, long ldw,
                                            long ldo, int v0, int vocab, int tile, hipStream_t s) {
  using namespace kgs::linear_xent;
  if (const int rc = check(h, w, target, T, Vc, K, ldh, ldw)) return rc;
  if (v0 < 0 || v0 % 128 || vocab % 128 || (long)v0 + Vc > vocab || ldo < Vc) return KGS_ERR_SHAPE;
  if (tile < -1 || tile > 1 || (tile == 1 && T % 256)) return KGS_ERR_ARG;
  if (!lse || !grow || !out || (uintptr_t)out % 16 || ldo % 8 || ((uintptr_t)lse | (uintptr_t)grow) % 4)
    return KGS_ERR_ALIGN;
  Args a = {};
  a.H = (const unsigned short*)h, a.W = (const unsigned short*)w, a.target = (const long long*)target;
  a.lse = lse, a.grow = grow, a.D = (unsigned short*)out;
  a.ldh = ldh, a.ldw = ldw, a.ldd = ldo, a.T = T, a.V = Vc, a.K = K, a.v0 = v0, a.vocab = vocab;
  if (tile < 0) tile = T % 256 == 0;
  return tile ? launch<4, 3, true>(a, s) : launch<2, 2, true>(a, s);
}
