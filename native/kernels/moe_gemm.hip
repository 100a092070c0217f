// Batched bf16 GEMM over mixture-of-experts capacity slabs (round 22).
//
// For every e in 0 .. E-1:  C_e[M, N] = A_e[M, K] . B_e[N, K]^T, bf16 in, fp32
// accumulation in ascending k, bf16 out rounded once. One launch covers all E
// products; leading dimensions (lda, ldb, ldc) and the per-e strides (sa, sb, sc,
// elements) are independent, so an operand may be a column block of a wider matrix.
//
// counts (device int32 [E], read by the kernel, never by the host) tells how much of
// slab e is filled, n_e = clamp(counts[e], 0, limit):
//   mode 0  no counts.
//   mode 1  rows, limit M: rows m >= n_e of C_e are stored as zeros whatever A_e holds
//           there; a tile wholly past n_e runs no K loop; a partly filled tile masks at
//           the store.
//   mode 2  reduction, limit K: only the K-steps of BK = 64 that start below n_e run, so
//           columns k >= roundup(n_e, 64) of both operands are never read; the columns in
//           [n_e, roundup(n_e, 64)) are read and the caller keeps them zero. n_e = 0
//           gives a zero C_e.
// Every element of C is written on every call (no memset in a captured step), there are
// no atomics, no workgroup waits on another, and the grid and the order of additions
// depend on the shapes and counts only: results are bitwise repeatable.
//
// Design. Tile BM x 128 with BM / 64 x 2 waves of 64 x 64 each: 16 accumulators of
// v_mfma_f32_16x16x32_bf16 (64 VGPRs) per wave, BK = 64. A and B K-tiles go HBM -> LDS by
// LDS-DMA in the lane-linear image of the project's GEMM: 128-byte rows, the 16-byte
// chunk c of row r stored at c ^ ((r >> 1) & 7), the XOR applied to the source address.
// NS stages; K-step t: wait for tile t, one barrier, read the 16 fragments of tile t,
// issue the DMA of tile t + NS - 1 into the stage tile t - 1 was read from (every wave
// finished those reads before it reached the barrier), 32 MFMAs. One barrier per K-step.
// Tile 1 = 256 x 128, 3 stages (144 KiB, one workgroup of 8 waves per CU, two K-tiles in
// flight): the faster shape on every slab measured (profiles/r22/moe_gemm/README.md), used
// whenever M % 256 == 0. Tile 0 = 128 x 128, 2 stages (64 KiB: two workgroups per CU, the
// second wave of a SIMD covers the barrier and the DMA wait) serves M % 256 == 128.
// 1-D static grid over (e, tile), one workgroup per tile: xcd_remap gives every XCD a
// contiguous range of logical ids, e = id / tiles-per-e, so the tiles of one e run on one
// XCD while B_e is in that L2; inside an e tiles go in groups of 8 tile-rows.
#include "kgs_common.h"

namespace kgs {
namespace moe_gemm {

constexpr int BN = 128, BK = 64, ROW = BK * 2, GROUP_M = 8;
enum { MODE_ALL = 0, MODE_ROWS = 1, MODE_REDUCE = 2 };

struct Args {
  const unsigned short* A;
  const unsigned short* B;
  unsigned short* C;
  const int* counts;
  long lda, ldb, ldc, sa, sb, sc;
  int M, N, K, mode;
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

template <int WM, int NS>
__global__ __launch_bounds__(WM * 128) void moe_gemm_nt(const Args p) {
  constexpr int BM = WM * 64, NW = WM * 2, NT = NW * 64;
  constexpr int A_BYTES = BM * ROW, STAGE = (BM + BN) * ROW;
  constexpr int RB = BN / NW;        // B rows a wave loads per K-tile
  constexpr int GA = 4, GB = RB / 8; // 1-KiB DMAs per wave per K-tile: 32 A rows, RB B rows
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int ntm = p.M / BM, ntn = p.N / BN, per_e = ntm * ntn;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int e = id / per_e, t = id - e * per_e;
  const int group = t / (GROUP_M * ntn), first = group * GROUP_M, in_group = t - group * GROUP_M * ntn;
  const int gsz = min(ntm - first, GROUP_M);
  const int tm = first + in_group % gsz, tn = in_group / gsz;

  int nt = p.K / BK, nrow = BM;  // K-steps to run, rows of this tile that are kept
  if (p.mode != MODE_ALL) {
    const int n = min(max(p.counts[e], 0), p.mode == MODE_ROWS ? p.M : p.K);
    if (p.mode == MODE_ROWS) nrow = min(n - tm * BM, BM); else nt = (n + BK - 1) / BK;
  }
  unsigned short* Ct = p.C + e * p.sc + (long)tm * BM * p.ldc + tn * BN;
  if (nrow <= 0 || nt == 0) {  // an empty tile: zeros, no K loop
    for (int i = threadIdx.x; i < BM * (BN / 8); i += NT)
      *(uint4*)(Ct + (long)(i >> 4) * p.ldc + (i & 15) * 8) = make_uint4(0, 0, 0, 0);
    return;
  }

  // DMA j of wave w fills rows w * 32 + j * 8 + lane / 8 of the A tile (w * RB + .. of
  // B); the lane's physical chunk lane & 7 holds logical chunk (lane & 7) ^ ((row >> 1) & 7)
  const unsigned short* pa[GA];
  const unsigned short* pb[GB];
  {
    const unsigned short* At = p.A + e * p.sa + (long)tm * BM * p.lda;
    const unsigned short* Bt = p.B + e * p.sb + (long)tn * BN * p.ldb;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const int r = w * 32 + j * 8 + (lane >> 3);
      pa[j] = At + r * p.lda + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int r = w * RB + j * 8 + (lane >> 3);
      pb[j] = Bt + r * p.ldb + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
    }
  }
  auto issue = [&](int stage, int k0) {
    char* dst = smem + stage * STAGE;
#pragma unroll
    for (int j = 0; j < GA; ++j) glds16(pa[j] + k0, dst + w * 4096 + j * 1024);
#pragma unroll
    for (int j = 0; j < GB; ++j) glds16(pb[j] + k0, dst + A_BYTES + w * (RB * ROW) + j * 1024);
  };

  // fragment reads: row lane & 15 of a 16-row block, logical chunk 4 s + lane / 16
  const int fr = lane & 15, fq = lane >> 4;
  const int ro0 = fr * ROW + ((fq ^ (fr >> 1)) * 16), ro1 = fr * ROW + (((4 + fq) ^ (fr >> 1)) * 16);
  const int offa = wr * 64 * ROW, offb = A_BYTES + wc * 64 * ROW;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < NS - 1; ++j)
    if (j < nt) issue(j, j * BK);

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
    if (kt + NS - 1 < nt) issue(ws, (kt + NS - 1) * BK);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          // B first: the lane ends up with 4 consecutive columns of one row,
          // C[i * 16 + (lane & 15)][n * 16 + 4 * (lane >> 4) + 0 .. 3]
          acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n][s], a[i][s], acc[i][n], 0, 0, 0);
    rs = rs + 1 == NS ? 0 : rs + 1;
    ws = ws + 1 == NS ? 0 : ws + 1;
  }

  // store: v_permlane16_swap pairs the n-tiles so that every lane writes 16 bytes; rows
  // at or past nrow (mode 1) are written as zeros
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = wr * 64 + i * 16 + fr;
    unsigned short* crow = Ct + (long)row * p.ldc + wc * 64;
    const bool keep = row < nrow;
#pragma unroll
    for (int np = 0; np < 2; ++np) {
      const f32x4 v0 = acc[i][2 * np], v1 = acc[i][2 * np + 1];
      const unsigned x0 = pack_bf16x2(v0[0], v0[1]), y0 = pack_bf16x2(v0[2], v0[3]);
      const unsigned x1 = pack_bf16x2(v1[0], v1[1]), y1 = pack_bf16x2(v1[2], v1[3]);
      const auto sx = __builtin_amdgcn_permlane16_swap(x0, x1, false, false);
      const auto sy = __builtin_amdgcn_permlane16_swap(y0, y1, false, false);
      // even fq: 8 consecutive columns of n-tile 2 np; odd fq: of n-tile 2 np + 1
      const uint4 q = keep ? make_uint4(sx[0], sy[0], sx[1], sy[1]) : make_uint4(0, 0, 0, 0);
      *(uint4*)(crow + np * 32 + (fq & 1) * 16 + (fq >> 1) * 8) = q;
    }
  }
}

template <int WM, int NS>
static int launch(const Args& a, int E, hipStream_t s) {
  const long grid = (long)E * (a.M / (WM * 64)) * (a.N / BN);
  if (a.M % (WM * 64) || grid > 0x7fffffffL) return KGS_ERR_SHAPE;
  hipLaunchKernelGGL((moe_gemm_nt<WM, NS>), dim3((unsigned)grid), dim3(WM * 128), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace moe_gemm
}  // namespace kgs

// tile: -1 in production = 256 x 128 x 3 stages where M % 256 == 0, else 128 x 128 x 2 stages;
// 0 / 1 force the one or the other for the A/B and the tests (1 needs M % 256 == 0). counts is required by modes 1 and 2 and ignored by mode 0.
KGS_EXPORT int kgs_moe_gemm_bf16_nt(const void* A, const void* B, void* C, const int* counts, int E, int M, int N,
                                    int K, long lda, long ldb, long ldc, long sa, long sb, long sc, int mode,
                                    int tile, hipStream_t s) {
  using namespace kgs::moe_gemm;
  if (E < 1 || M < 128 || N < 128 || K < 64 || M % 128 || N % 128 || K % 64) return KGS_ERR_SHAPE;
  if (lda < K || ldb < K || ldc < N || sa < 0 || sb < 0 || sc < 0) return KGS_ERR_SHAPE;
  if (E > 1 && sc < (long)M * ldc) return KGS_ERR_SHAPE;  // output slabs may not overlap (inputs may)
  if (mode < MODE_ALL || mode > MODE_REDUCE || tile < -1 || tile > 1 || (mode != MODE_ALL && !counts)) return KGS_ERR_ARG;
  if (!A || !B || !C || ((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) % 16 || (uintptr_t)counts % 4 ||
      (lda | ldb | ldc | sa | sb | sc) % 8)
    return KGS_ERR_ALIGN;
  const Args a = {(const unsigned short*)A, (const unsigned short*)B, (unsigned short*)C,
                  mode == MODE_ALL ? nullptr : counts, lda, ldb, ldc, sa, sb, sc, M, N, K, mode};
  if (tile < 0) tile = M % 256 == 0;
  return tile ? launch<4, 3>(a, E, s) : launch<2, 2>(a, E, s);
}
