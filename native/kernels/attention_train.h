// What the training attention files share: attention_train.hip (head_dim 128,
// causal or full), attention_window.hip (head_dim 128, sliding window) and
// attention_d64.hip (head_dim 64). Each mechanism is described here, once.
//
//   * for any head_dim: the kernel arguments, the delta pass, the accumulator
//     store, the inline-asm transposed reads, the dispatch swizzle, and the
//     host-side argument checks and three-stage backward launch;
//   * for head_dim 128 (the 64 x 128 tile in the XOR image of attention_fwd.h):
//     the transposed-read addresses and the K | V tile-pair LDS-DMA.
//
// The compute kernels themselves stay in their files. One bwd_dkdv body and one
// bwd_dq body for attn_train and attn_win under a mask policy were built and
// measured; hipcc compiled neither to the streams the kernels have, and the
// merged bodies missed the timing margin or spilled
// (profiles/r20/attention_shared/README.md), so each file keeps its own.
#pragma once
#include "attention_fwd.h"

namespace kgs {
namespace attn {

constexpr float LOG2E = 1.4426950408889634f;

// One layout for every forward / backward kernel of the three files. `mask` is
// the causal flag (0 / 1) in attn_train and attn64, the window W (1 <= W <= S)
// in attn_win.
struct FwdArgs {
  const unsigned short* q;
  const unsigned short* k;
  const unsigned short* v;
  unsigned short* o;
  float* lse;               // fp32 [B*H, S], natural log (fwd<true> only)
  long ldq, ldk, ldv, ldo;  // row strides (elements)
  int B, S, H, HKV;
  float sl2;  // softmax scale * log2(e)
  int mask;
};

struct BwdArgs {
  const unsigned short* q;
  const unsigned short* k;
  const unsigned short* v;
  const unsigned short* o;
  const unsigned short* dout;
  const float* lse;  // [B*H, S]
  float* delta;      // [B*H, S] workspace
  unsigned short* dq;
  unsigned short* dk;
  unsigned short* dv;
  long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;  // row strides (elements)
  int B, S, H, HKV;
  float scale, sl2;  // softmax scale, scale * log2(e)
  int mask;
};

// XCD-aware dispatch order: 8 consecutive dispatch slots of one XCD take 4
// heads of one KV group, so the K/V tiles they share are L2 hits.
__device__ __forceinline__ int dispatch_id(int bid, int nwg) {
  if (nwg & 31) return bid;
  const int t = bid >> 3, x = bid & 7;
  return ((t >> 2) << 5) | (x << 2) | (t & 3);
}

// delta[b H + h, s] = sum_d dO[b s, h, d] O[b s, h, d]: D / 8 lanes x 8
// elements per (token, head), summed in-lane and then by a fixed xor tree.
template <int D>
__device__ __forceinline__ void prep_body(const BwdArgs& a) {
  constexpr int LANES = D / 8;
  const long item = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES;  // (token, head)
  const long total = (long)a.B * a.S * a.H;
  const int part = threadIdx.x % LANES;
  float acc = 0.f;
  long tok = 0;
  int h = 0;
  if (item < total) {
    tok = item / a.H;
    h = (int)(item - tok * a.H);
    const uint4 x = *(const uint4*)(a.o + tok * a.ldo + (long)h * D + 8 * part);
    const uint4 y = *(const uint4*)(a.dout + tok * a.lddo + (long)h * D + 8 * part);
    const unsigned xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc = __builtin_fmaf(bf2f((unsigned short)(xs[i] & 0xffff)), bf2f((unsigned short)(ys[i] & 0xffff)), acc);
      acc = __builtin_fmaf(bf2f((unsigned short)(xs[i] >> 16)), bf2f((unsigned short)(ys[i] >> 16)), acc);
    }
  }
#pragma unroll
  for (int s = LANES / 2; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, LANES);
  if (item < total && part == 0) {
    const long b = tok / a.S, srow = tok - b * a.S;
    a.delta[(b * a.H + h) * a.S + srow] = acc;
  }
}

// acc (rows (r&3) + 8 (r>>2) + 4 hh of a 32-row block on the registers, the
// lane's column on l32) x mul -> the 32 N bf16 columns of the lane's row.
template <int N>
__device__ __forceinline__ void store_acc_row(unsigned short* rowp, const f32x16 (&acc)[N], int hh, float mul = 1.0f) {
#pragma unroll
  for (int d = 0; d < N; ++d)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      uint2 pk;
      pk.x = pack_bf16x2(acc[d][4 * r4 + 0] * mul, acc[d][4 * r4 + 1] * mul);
      pk.y = pack_bf16x2(acc[d][4 * r4 + 2] * mul, acc[d][4 * r4 + 3] * mul);
      *(uint2*)(rowp + 32 * d + 8 * r4 + 4 * hh) = pk;
    }
}

// A transposed fragment (tr_frag of attention_fwd.h) by inline-asm reads, for a
// loop that keeps an LDS-DMA in flight: hipcc puts a vmcnt(0) before a BUILTIN
// ds_read_tr then (its LDS-DMA alias check), which drains the DMA, and a lone
// wave per SIMD cannot hide that (docs/architecture.md, "LDS-DMA alias waits").
// The caller orders the DMA before these reads (its own vmcnt + barrier) and
// retires them with tr_wait before use. lo / hi: the lane's LDS addresses of
// the low and the high four k; they belong to the tile geometry.
struct TrPair {
  bf16x4s lo, hi;
};
__device__ __forceinline__ TrPair tr_read_asm(const char* lo, const char* hi) {
  const unsigned a0 = (unsigned)(uintptr_t)(const KGS_LDS char*)lo;
  const unsigned a1 = (unsigned)(uintptr_t)(const KGS_LDS char*)hi;
  TrPair r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r.lo) : "v"(a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r.hi) : "v"(a1));
  return r;
}
// lgkmcnt(0) tied to the N fragments read above: every use of them depends on
// this statement, so no consumer can be scheduled ahead of the wait
template <int N>
__device__ __forceinline__ void tr_wait(TrPair (&f)[N]) {
  static_assert(N == 4 || N == 8, "one asm statement per fragment count");
#define KGS_TR_TIE(i) "+v"(f[i].lo), "+v"(f[i].hi)
  if constexpr (N == 4)
    asm volatile("s_waitcnt lgkmcnt(0)" : KGS_TR_TIE(0), KGS_TR_TIE(1), KGS_TR_TIE(2), KGS_TR_TIE(3));
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : KGS_TR_TIE(0), KGS_TR_TIE(1), KGS_TR_TIE(2), KGS_TR_TIE(3), KGS_TR_TIE(4), KGS_TR_TIE(5),
                   KGS_TR_TIE(6), KGS_TR_TIE(7));
#undef KGS_TR_TIE
}
__device__ __forceinline__ bf16x8 tr_join(const TrPair& f) {
  return __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- head_dim 128: the 64 x 128 tile of attention_fwd.h ----

constexpr int KBW = 128;  // keys per bwd_dkdv workgroup (4 waves x 32)

// X^T fragments (A operand) of rows rb .. rb+15 x columns 32 d + l32 of a tile,
// in the k order of an accumulator used as the B operand (row = rb + 8 (e>>2) +
// 4 hh + (e&3) for element e): the low four k from row rb + 4 hh + tq, the high
// four from 8 below. By builtin reads (tr_rows) or asm reads (tr_rows_asm);
// each spells the addresses out: with a shared address helper hipcc spills 5
// VGPRs in attn_win::bwd_dq, which sits at 256 (profiles/r20/attention_shared).
__device__ __forceinline__ bf16x8 tr_rows(const char* tile, int rb, int d, int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3, hh = lane >> 5;
  const int c0 = 4 * d + 2 * (g & 1) + (tp >> 1);
  const int row = rb + 4 * hh + tq;
  return tr_frag(tile + off(row, c0) + 8 * (tp & 1), tile + off(row + 8, c0) + 8 * (tp & 1));
}
__device__ __forceinline__ TrPair tr_rows_asm(const char* tile, int rb, int d, int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3, hh = lane >> 5;
  const int c0 = 4 * d + 2 * (g & 1) + (tp >> 1);
  const int row = rb + 4 * hh + tq;
  return tr_read_asm(tile + off(row, c0) + 8 * (tp & 1), tile + off(row + 8, c0) + 8 * (tp & 1));
}

// Two 64-row tiles (K and V), rows 64 jt .. 64 jt + 63 of x and of y, -> LDS
// [x tile | y tile] at sb by LDS-DMA (global_load_lds, no staging registers): a
// 16 KB tile is 16 chunks of 1 KB = 4 rows of 256 B, wave w issues chunks
// 4w .. 4w+3 of each. Lane l lands at chunk + 16 l, i.e. at slot (r, c') of the
// XOR image, so it fetches column c = c' ^ swz(r). The window forward and
// bwd_dq call it; the kernels that spell the same loop out are listed with
// the reason in profiles/r20/attention_shared/README.md.
__device__ __forceinline__ void dma_pair(const unsigned short* x, const unsigned short* y, long ldx, long ldy, int jt,
                                         char* sb, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = 4 * w + i;
    const int r = 4 * ch + (lane >> 4), c = (lane & 15) ^ swz(r);
    const long row = (long)jt * KB + r;
    glds16(x + row * ldx + 8 * c, sb + 1024 * ch);
    glds16(y + row * ldy + 8 * c, sb + TILE_BYTES + 1024 * ch);
  }
}

// ---- host side ----

// The argument checks of a forward entry, in the order the entries report
// them: dimensions, then `mode_err` (the entry's verdict on its own mode
// arguments, 0 if fine), strides, pointers. A is FwdArgs or attn::Args; D is
// the kernels' head_dim. lse may be null unless need_lse. Returns 0 or KGS_ERR_*.
template <class A>
inline int check_fwd(const A& a, const void* lse, bool need_lse, int hd, int D, int mode_err) {
  if (a.B <= 0 || a.S <= 0 || a.H <= 0 || a.HKV <= 0 || a.H % a.HKV) return KGS_ERR_SHAPE;
  if (hd != D || a.S % QB) return KGS_ERR_SHAPE;
  if (mode_err) return mode_err;
  const long qc = (long)a.H * D, kc = (long)a.HKV * D;
  if (a.ldq < qc || a.ldk < kc || a.ldv < kc || a.ldo < qc) return KGS_ERR_SHAPE;
  if (!a.q || !a.k || !a.v || !a.o || (need_lse && !lse)) return KGS_ERR_ALIGN;
  const uintptr_t al = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.o | (uintptr_t)lse;
  if ((al & 15) || (a.ldq | a.ldk | a.ldv | a.ldo) & 7) return KGS_ERR_ALIGN;
  if ((long)a.B * a.H * (a.S / QB) > 0x7fffffff) return KGS_ERR_SHAPE;  // the grid
  return KGS_OK;
}

// The same for a backward entry; every pointer is required.
inline int check_bwd(const BwdArgs& a, int hd, int D, int mode_err) {
  if (a.B <= 0 || a.S <= 0 || a.H <= 0 || a.HKV <= 0 || a.H % a.HKV) return KGS_ERR_SHAPE;
  if (hd != D || a.S % QB) return KGS_ERR_SHAPE;
  if (mode_err) return mode_err;
  const long qc = (long)a.H * D, kc = (long)a.HKV * D;
  if (a.ldq < qc || a.ldo < qc || a.lddo < qc || a.lddq < qc || a.ldk < kc || a.ldv < kc || a.lddk < kc || a.lddv < kc)
    return KGS_ERR_SHAPE;
  if (!a.q || !a.k || !a.v || !a.o || !a.dout || !a.lse || !a.delta || !a.dq || !a.dk || !a.dv) return KGS_ERR_ALIGN;
  const uintptr_t al = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.o | (uintptr_t)a.dout |
                       (uintptr_t)a.lse | (uintptr_t)a.delta | (uintptr_t)a.dq | (uintptr_t)a.dk | (uintptr_t)a.dv;
  if ((al & 15) || (a.ldq | a.ldk | a.ldv | a.ldo | a.lddo | a.lddq | a.lddk | a.lddv) & 7) return KGS_ERR_ALIGN;
  if (((long)a.B * a.S * a.H * (D / 8) + 255) / 256 > 0x7fffffff) return KGS_ERR_SHAPE;  // bwd_prep's grid
  return KGS_OK;
}

// The three backward launches of checked arguments. stages: bit 0 bwd_prep
// (D / 8 lanes per (token, head)), bit 1 bwd_dkdv (kbw keys per workgroup),
// bit 2 bwd_dq (QB rows per workgroup); the benchmarks time them apart.
// Allocates nothing and synchronises nothing.
using BwdKernel = void (*)(BwdArgs);
inline int launch_bwd(BwdKernel prep, BwdKernel dkdv, BwdKernel dq, const BwdArgs& a, int D, int kbw, int stages,
                      hipStream_t s) {
  const long nprep = ((long)a.B * a.S * a.H * (D / 8) + 255) / 256;
  const long nkv = (long)a.B * a.HKV * (a.S / kbw), ndq = (long)a.B * a.H * (a.S / QB);
  if (stages & 1) hipLaunchKernelGGL(prep, dim3((unsigned)nprep), dim3(256), 0, s, a);
  if (stages & 2) hipLaunchKernelGGL(dkdv, dim3((unsigned)nkv), dim3(256), 0, s, a);
  if (stages & 4) hipLaunchKernelGGL(dq, dim3((unsigned)ndq), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace attn
}  // namespace kgs
