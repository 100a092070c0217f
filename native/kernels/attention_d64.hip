// Flash-attention for training at head_dim 64 on gfx950: the forward (with or
// without each query row's log-sum-exp) and the backward (dQ, dK, dV) that
// recomputes P from it. The contract is that of the head_dim 128 training
// kernels (attention_train.hip): bf16 in/out, fp32 softmax/accumulate, causal or
// full, GQA, Sk == S, S % 128 == 0, token-major operands with any row stride (a
// multiple of 8), so q/k/v and dq/dk/dv can be the three column groups of a
// fused QKV / dQKV buffer. No atomics, no workgroup waits on another, every sum
// has a fixed order (bitwise repeatable, capturable in a graph); P and dS are
// rounded to bf16 once, as MFMA operands.
//
//   P = exp2(c S - lse log2 e), c = scale log2 e     delta = rowsum(dO o O)
//   dV = P^T dO     dP = dO V^T     dS = scale P o (dP - delta)
//   dQ = dS K       dK = dS^T Q
//
// These are not the 128 kernels with a constant changed. Per key the softmax
// work is the same while the MFMA work and the accumulators halve, so the
// registers that frees go to a longer tile: every staged tile is 128 rows x 64
// columns (16 KB, as many LDS-DMA issues per wave as a 64 x 128 tile) and
// barriers and loop overhead per key halve.
//
// LDS image. A tile row is 128 B = 8 chunks of 16 B; chunk c of row r sits at
//     off(r, c) = 128 r + 16 (c ^ swz(r)),   swz(r) = ((r >> 1) & 1) << 2 | ((r >> 2) & 3)
// and the XOR is applied to the LDS-DMA's per-lane SOURCE column. LDS has 64
// banks x 4 B, i.e. 16 "slots" of 16 B per 256 B; a slot index is
// 8 (r & 1) + (c ^ swz(r)). An access is conflict-free when the lanes served
// together cover 256 B in 16 distinct slots:
//   * row reads (ds_read_b128, 16 lanes together): rows r0 .. r0+15 (r0 % 16 ==
//     0) of one chunk c. Each parity class r = p + 2 i, i = 0..7, has swz =
//     4 (i & 1) + (i >> 1), a bijection on 0..7, so its 8 rows take the 8 slots
//     of their half; the two parities take the two halves.
//   * transposed reads (ds_read_b64_tr_b16, 32 lanes x 8 B together): rows
//     r0 .. r0+3 (r0 % 4 == 0) x the 4 chunks 4 d .. 4 d + 3. Rows r0 and r0+2
//     (same parity) have swz x and 4 + x (x = (r0 >> 2) & 3): the first keeps the
//     chunks in their aligned group of four, the second moves them to the other
//     group, so the 8 slots of that half are each taken once; rows r0+1 and
//     r0+3 do the same in the other half. The two 8-B halves of a chunk are
//     read by two lanes of the same access and share its slot without conflict.
//
//   * fwd<LSE>: one workgroup = 4 waves x 32 query rows of one (q-block, head),
//     2 workgroups per CU. Swapped QK^T (S^T = K Q^T, a lane owns one query
//     row), the S^T accumulator is the B operand of O^T += V^T P^T, V^T by
//     transposed reads, K/V double buffer by LDS-DMA, row max by xor32_max,
//     deferred running-max rescale. Per lane: 4 S accumulators (64 registers),
//     2 O accumulators (32), 16 K fragments, 4 Q fragments. Under the causal
//     mask the diagonal tile spans the whole q-block, so wave w computes only
//     its first w + 1 sub-blocks of 32 keys (a wave-uniform decision) and masks
//     only the last of them. Dispatch is XCD aware, heaviest q-blocks first.
//   * bwd_prep: delta[b H + h, s] (fp32): 8 lanes x 8 elements per (token,
//     head), a fixed xor tree.
//   * bwd_dkdv: one workgroup = 4 waves x 32 keys of one (batch, KV head); a
//     wave keeps its keys' K and V fragments (4 + 4) and the dK^T / dV^T
//     accumulators (2 + 2) in registers while the workgroup sweeps the group's
//     query heads x 128-row Q / dO tiles (with their lse and delta) that arrive
//     by LDS-DMA. The key is on the MFMA lane, so the P and dS accumulators are
//     the B operands of dV^T += dO^T P and dK^T += Q^T dS. The transposed reads
//     are inline asm behind the loop's own vmcnt + barrier: nothing inside a
//     tile waits on vector memory (docs/architecture.md, "LDS-DMA alias
//     waits"). Causal: only tiles at or after the key block are swept, a wave
//     skips the 32-row sub-blocks wholly before its keys, key blocks dispatch
//     heaviest first.
//   * bwd_dq: the mirror of the forward. A lane owns one query row (Q and dO
//     fragments, lse and delta in registers), S^T = K Q^T, dP^T = V dO^T,
//     dQ^T += K^T dS^T with dS^T straight from the accumulator; the forward's
//     128-key tile and per-sub-block causal skip. No softmax couples the
//     sub-blocks here, so each is finished before the next starts.
#include "attention_train.h"

namespace kgs {
namespace attn64 {

using attn::bf16x4s;
using attn::BwdArgs;
using attn::dispatch_id;
using attn::f32x16;
using attn::FwdArgs;
using attn::LOG2E;
using attn::store_acc_row;
using attn::tr_join;
using attn::tr_wait;
using attn::TrPair;
// BwdArgs / FwdArgs::mask is the causal flag (0 / 1) in this file

constexpr int HD = 64;
constexpr int QB = 128;  // query rows per workgroup (4 waves x 32)
constexpr int KB = 128;  // rows per staged tile
constexpr int TILE_BYTES = KB * HD * 2;  // 16 KB
constexpr float NEG = -1.0e30f;
constexpr float RESCALE = 8.0f;  // deferred-max threshold, log2 units: P <= 256
static_assert(QB == attn::QB, "attention_train.h checks S against the 128 kernels' q-block");

__device__ __forceinline__ int swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int off(int r, int c) { return 128 * r + 16 * (c ^ swz(r)); }

template <bool V>
struct Flag {
  static constexpr bool value = V;
};

// One 128 x 64 tile -> LDS by LDS-DMA: 16 chunks of 1 KB = 8 rows of 128 B; wave
// w issues chunks 4w .. 4w+3. Lane l lands at chunk + 16 l, i.e. at slot
// (r, c') of the XOR image, so it fetches column chunk c = c' ^ swz(r).
__device__ __forceinline__ void dma_tile(const unsigned short* base, long ld, char* dst, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = 4 * w + i;
    const int r = 8 * ch + (lane >> 3), c = (lane & 7) ^ swz(r);
    glds16(base + (long)r * ld + 8 * c, dst + 1024 * ch);
  }
}

// Lane addresses of X^T fragments (A operand) of rows rb .. rb+15 x columns
// 32 d + l32 of a tile, in the k order of an accumulator used as the B operand
// (register 8 s + j of a 32 x 32 accumulator is row 16 s + 8 (j >> 2) + 4 hh +
// (j & 3)): the low four k from row rb + 4 hh + tq, the high four from 8 below.
__device__ __forceinline__ int tr_off(int rb, int d, int lane, int hi) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3, hh = lane >> 5;
  return off(rb + 4 * hh + tq + 8 * hi, 4 * d + 2 * (g & 1) + (tp >> 1)) + 8 * (tp & 1);
}
__device__ __forceinline__ bf16x8 tr_rows(const char* tile, int rb, int d, int lane) {
  const bf16x4s a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((KGS_LDS bf16x4s*)(tile + tr_off(rb, d, lane, 0)));
  const bf16x4s b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((KGS_LDS bf16x4s*)(tile + tr_off(rb, d, lane, 1)));
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The same fragment by asm reads (attention_train.h), for bwd_dkdv's loop
__device__ __forceinline__ TrPair tr_rows_asm(const char* tile, int rb, int d, int lane) {
  return attn::tr_read_asm(tile + tr_off(rb, d, lane, 0), tile + tr_off(rb, d, lane, 1));
}

template <bool LSE>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void fwd(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2][2][TILE_BYTES];  // [buf][K, V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int nqb = a.S / QB;
  const int lid = dispatch_id(blockIdx.x, gridDim.x);
  const int per = a.B * a.H;
  const int qi = lid / per, rem = lid - qi * per;
  const int qb = a.mask ? nqb - 1 - qi : qi;
  const int b = rem / a.H, h = rem - b * a.H;
  const int kvh = h / (a.H / a.HKV);

  const int qrow = qb * QB + 32 * w + l32;  // this lane's query row
  const long tok0 = (long)b * a.S;

  // Q fragments (B operand of S^T = K.Q^T): lane holds Q[qrow][16ks + 8hh .. +7]
  bf16x8 qf[4];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (tok0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qp[2 * ks];
  }

  const unsigned short* kbase = a.k + tok0 * a.ldk + (long)kvh * HD;
  const unsigned short* vbase = a.v + tok0 * a.ldv + (long)kvh * HD;
  auto dma_tiles = [&](int jn, int sb) {
    dma_tile(kbase + (long)jn * KB * a.ldk, a.ldk, smem[sb][0], w, lane);
    dma_tile(vbase + (long)jn * KB * a.ldv, a.ldv, smem[sb][1], w, lane);
  };

  const int ntile = a.mask ? qb + 1 : a.S / KB;
  dma_tiles(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the Q fragments and tile 0
  __syncthreads();

  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) o[d] = f32x16{};
  float m = NEG, l = 0.f;
  const float sl2 = a.sl2;

  // One tile. DIAG: the causal diagonal tile (its keys are the q-block's own
  // rows), of which this wave sees sub-blocks 0 .. nt-1 = w and masks the last.
  auto tile = [&](auto diag_c, const int nt, const char* Ks, const char* Vs) {
    constexpr bool DIAG = decltype(diag_c)::value;
    // all K fragments of the tile are read up front, so the QK^T MFMAs never
    // wait on one LDS read
    bf16x8 kf[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (!DIAG || t < nt) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[t][ks] = *(const bf16x8*)(Ks + off(32 * t + l32, 2 * ks + hh));
      }
    __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead (the scheduler sinks them otherwise)
    f32x16 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (!DIAG || t < nt) {
        s[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[t][ks], qf[ks], s[t], 0, 0, 0);
      }
    // the first half of the V fragments is read now, so its LDS latency hides
    // under the softmax; the second half is read under the first half's MFMAs
    bf16x8 vfr[2][4][2];
    auto read_v = [&](int d) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (!DIAG || t < nt) {
#pragma unroll
          for (int sp = 0; sp < 2; ++sp) vfr[d][t][sp] = tr_rows(Vs, 32 * t + 16 * sp, d, lane);
        }
    };
    read_v(0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DIAG) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t == nt - 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((r & 3) + 8 * (r >> 2) + 4 * hh > l32) s[t][r] = NEG;
        }
    }
    float mx = m;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (!DIAG || t < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
      }
    mx = xor32_max(mx);
    // deferred rescale: the running max m only moves when a row's new max
    // exceeds it by more than RESCALE (log2 units after sl2), so most tiles
    // skip the O rescale; p = exp2(s sl2 - m sl2) stays <= 2^RESCALE. Both l
    // and O see the same alpha, and the decision is wave-uniform.
    const bool grow = (mx - m) * sl2 > RESCALE;
    if (__any(grow)) {
      const float mn = grow ? mx : m;
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * sl2);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int d = 0; d < 2; ++d) o[d] *= alpha;
    }
    const float msl = m * sl2;
    bf16x8 pf[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (!DIAG || t < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -msl));
          s[t][r] = p;
          l += p;
        }
        pf[t][0] = pack_bf16x8(s[t], 0);
        pf[t][1] = pack_bf16x8(s[t], 8);
      }
    read_v(1);
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (!DIAG || t < nt) {
#pragma unroll
          for (int sp = 0; sp < 2; ++sp)
            o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[d][t][sp], pf[t][sp], o[d], 0, 0, 0);
        }
  };

  // the causal diagonal tile is the last one: it runs after the loop, so the
  // loop body is straight-line code
  const int nfull = a.mask ? qb : ntile;
  for (int j = 0; j < nfull; ++j) {
    const int buf = j & 1;
    // the other buffer was released by the previous tile's barrier
    if (j + 1 < ntile) dma_tiles(j + 1, buf ^ 1);
    tile(Flag<false>{}, 4, smem[buf][0], smem[buf][1]);
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }
  if (a.mask) tile(Flag<true>{}, w + 1, smem[nfull & 1][0], smem[nfull & 1][1]);

  l = xor32_sum(l);
  if constexpr (LSE) {
    // ln sum exp(scale s) = (m sl2 + log2 l) ln 2; the 32 lanes of a half-wave
    // write 32 consecutive floats
    if (hh == 0)
      a.lse[((long)b * a.H + h) * a.S + qrow] = (m * sl2 + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
  }
  store_acc_row(a.o + (tok0 + qrow) * a.ldo + (long)h * HD, o, hh, 1.0f / l);
}

__global__ __launch_bounds__(256) void bwd_prep(BwdArgs a) { attn::prep_body<HD>(a); }

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void bwd_dkdv(BwdArgs a) {
  // [buf][Q | dO (128 query rows each) | their lse | their delta]
  constexpr int ROWS_OFF = 2 * TILE_BYTES, BUF_BYTES = ROWS_OFF + 1024;
  __shared__ __attribute__((aligned(16))) char smem[2][BUF_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int G = a.H / a.HKV;
  // key blocks in dispatch order: block 0 sees every query tile under the
  // causal mask, so ascending order is heaviest first
  const int per = a.B * a.HKV;
  const int kbi = blockIdx.x / per, rem = blockIdx.x - kbi * per;
  const int b = rem / a.HKV, kvh = rem - b * a.HKV;
  const int key = kbi * KB + 32 * w + l32;  // this lane's key
  const long tok0 = (long)b * a.S;

  // K and V fragments (B operands of S = Q.K^T and dP = dO.V^T): lane holds
  // K[key][16 ks + 8 hh .. +7]
  bf16x8 kf[4], vf[4];
  {
    const bf16x8* kp = (const bf16x8*)(a.k + (tok0 + key) * a.ldk + (long)kvh * HD + 8 * hh);
    const bf16x8* vp = (const bf16x8*)(a.v + (tok0 + key) * a.ldv + (long)kvh * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = kp[2 * ks];
      vf[ks] = vp[2 * ks];
    }
  }

  const int nqt = a.S / KB;              // 128-row query tiles per head
  const int qt0 = a.mask ? kbi : 0;      // first tile that sees this key block (mask: the causal flag)
  const int nper = nqt - qt0;
  const int niter = G * nper;

  // the next tile to fetch: query tile qt0 + qn of head hn
  int qn = 0, hn = kvh * G;
  auto dma_tiles = [&](int sb) {
    const int qt = qt0 + qn, h = hn;
    if (++qn == nper) {
      qn = 0;
      ++hn;
    }
    dma_tile(a.q + (tok0 + (long)qt * KB) * a.ldq + (long)h * HD, a.ldq, smem[sb], w, lane);
    dma_tile(a.dout + (tok0 + (long)qt * KB) * a.lddo + (long)h * HD, a.lddo, smem[sb] + TILE_BYTES, w, lane);
    // the tile's 128 lse and 128 delta values (512 B each) ride along: lanes
    // 0-31 fetch lse, 32-63 delta
    if (w == 0) {
      const long rowoff = ((long)b * a.H + h) * a.S + (long)qt * KB;
      glds16((hh ? a.delta : a.lse) + rowoff + 4 * l32, smem[sb] + ROWS_OFF);
    }
  };

  dma_tiles(0);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): K/V fragments and tile 0
  __syncthreads();

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    dk[d] = f32x16{};
    dv[d] = f32x16{};
  }
  const float sl2 = a.sl2;

  for (int it = 0, qc = 0; it < niter; ++it) {
    const int buf = it & 1;
    // the other buffer was released by the previous iteration's barrier
    if (it + 1 < niter) dma_tiles(buf ^ 1);
    const char* Qs = smem[buf];
    const char* Ds = smem[buf] + TILE_BYTES;
    const char* Ls = smem[buf] + ROWS_OFF;
    // the diagonal tile holds the key block's own rows: sub-blocks before this
    // wave's keys see none of them, the wave's own sub-block is masked
    const bool diag = a.mask && qc == 0;
    if (++qc == nper) qc = 0;
    const int t0 = diag ? w : 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t >= t0) {
        f32x16 s = f32x16{}, dp = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 qa = *(const bf16x8*)(Qs + off(32 * t + l32, 2 * ks + hh));
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 da = *(const bf16x8*)(Ds + off(32 * t + l32, 2 * ks + hh));
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], dp, 0, 0, 0);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          // register 4 r4 + i is query row 32 t + 8 r4 + 4 hh + i of the tile
          const int qr = 32 * t + 8 * r4 + 4 * hh;
          const f32x4 ls = *(const f32x4*)(Ls + 4 * qr);
          const f32x4 de = *(const f32x4*)(Ls + 512 + 4 * qr);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * r4 + i;
            s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sl2, -ls[i] * LOG2E));
            dp[r] -= de[i];
          }
        }
        if (diag && t == w) {
          // the wave's own sub-block: keys after the query row see nothing. The
          // opaque copy keeps the 16 compares here; hoisted out of the loop
          // they are 16 lane masks in scalar registers, which then spill.
          int thr = l32 - 4 * hh;
          asm volatile("" : "+v"(thr));
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (thr > (r & 3) + 8 * (r >> 2)) s[r] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] *= s[r];
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const bf16x8 pf = pack_bf16x8(s, 8 * sp), dsf = pack_bf16x8(dp, 8 * sp);
          TrPair f[4];  // dO^T (0-1) and Q^T (2-3) of these 16 query rows
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            f[d] = tr_rows_asm(Ds, 32 * t + 16 * sp, d, lane);
            f[2 + d] = tr_rows_asm(Qs, 32 * t + 16 * sp, d, lane);
          }
          tr_wait(f);
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_join(f[d]), pf, dv[d], 0, 0, 0);
            dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_join(f[2 + d]), dsf, dk[d], 0, 0, 0);
          }
        }
      }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }

  // dS = scale P o (dP - delta): the scale is applied once, to the fp32 sum
  store_acc_row(a.dk + (tok0 + key) * a.lddk + (long)kvh * HD, dk, hh, a.scale);
  store_acc_row(a.dv + (tok0 + key) * a.lddv + (long)kvh * HD, dv, hh);
}

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void bwd_dq(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2][2][TILE_BYTES];  // [buf][K, V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int nqb = a.S / QB;
  const int lid = dispatch_id(blockIdx.x, gridDim.x);  // the forward's order
  const int per = a.B * a.H;
  const int qi = lid / per, rem = lid - qi * per;
  const int qb = a.mask ? nqb - 1 - qi : qi;
  const int b = rem / a.H, h = rem - b * a.H;
  const int kvh = h / (a.H / a.HKV);

  const int qrow = qb * QB + 32 * w + l32;  // this lane's query row
  const long tok0 = (long)b * a.S;

  // Q and dO fragments (B operands of S^T = K.Q^T and dP^T = V.dO^T)
  bf16x8 qf[4], dof[4];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (tok0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
    const bf16x8* dp_ = (const bf16x8*)(a.dout + (tok0 + qrow) * a.lddo + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = qp[2 * ks];
      dof[ks] = dp_[2 * ks];
    }
  }
  const long srow = ((long)b * a.H + h) * a.S + qrow;
  const float lse2 = a.lse[srow] * LOG2E;
  const float delta = a.delta[srow];

  const unsigned short* kbase = a.k + tok0 * a.ldk + (long)kvh * HD;
  const unsigned short* vbase = a.v + tok0 * a.ldv + (long)kvh * HD;
  auto dma_tiles = [&](int jn, int sb) {
    dma_tile(kbase + (long)jn * KB * a.ldk, a.ldk, smem[sb][0], w, lane);
    dma_tile(vbase + (long)jn * KB * a.ldv, a.ldv, smem[sb][1], w, lane);
  };

  const int ntile = a.mask ? qb + 1 : a.S / KB;
  dma_tiles(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the fragments, lse, delta and tile 0
  __syncthreads();

  f32x16 dq[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) dq[d] = f32x16{};
  const float sl2 = a.sl2;

  // One tile: the sub-blocks of 32 keys one after another. DIAG: the causal
  // diagonal tile, of which this wave sees sub-blocks 0 .. w and masks the last.
  auto tile = [&](auto diag_c, const char* Ks, const char* Vs) {
    constexpr bool DIAG = decltype(diag_c)::value;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (!DIAG || t <= w) {
        f32x16 s = f32x16{}, dp = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 ka = *(const bf16x8*)(Ks + off(32 * t + l32, 2 * ks + hh));
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[ks], s, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 va = *(const bf16x8*)(Vs + off(32 * t + l32, 2 * ks + hh));
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, dof[ks], dp, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sl2, -lse2));
          if (DIAG && t == w && (r & 3) + 8 * (r >> 2) + 4 * hh > l32) p = 0.f;
          dp[r] = p * (dp[r] - delta);
        }
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const bf16x8 dsf = pack_bf16x8(dp, 8 * sp);
#pragma unroll
          for (int d = 0; d < 2; ++d)
            dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_rows(Ks, 32 * t + 16 * sp, d, lane), dsf, dq[d], 0, 0, 0);
        }
      }
  };

  // the causal diagonal tile is the last one and runs after the loop
  const int nfull = a.mask ? qb : ntile;
  for (int j = 0; j < nfull; ++j) {
    const int buf = j & 1;
    if (j + 1 < ntile) dma_tiles(j + 1, buf ^ 1);
    tile(Flag<false>{}, smem[buf][0], smem[buf][1]);
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }
  if (a.mask) tile(Flag<true>{}, smem[nfull & 1][0], smem[nfull & 1][1]);

  store_acc_row(a.dq + (tok0 + qrow) * a.lddq + (long)h * HD, dq, hh, a.scale);
}

}  // namespace attn64
}  // namespace kgs

// Attention forward at head_dim 64. q/k/v/o point at head 0 of token 0
// ([B*S, ld] token-major); heads of one token are contiguous 64-element blocks.
// Requires S % 128 == 0, H % HKV == 0, 16-B aligned pointers and ld % 8 == 0.
// lse: fp32 [B*H, S] (natural log) or null; the output bits do not depend on it.
KGS_EXPORT int kgs_attn64_fwd_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int S, int H,
                                  int HKV, long ldq, long ldk, long ldv, long ldo, float scale, int causal,
                                  hipStream_t s) {
  using namespace kgs::attn64;
  const FwdArgs a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)o,
                  (float*)lse, ldq, ldk, ldv, ldo, B, S, H, HKV, scale * LOG2E, causal ? 1 : 0};
  // this entry has no head_dim argument: the hd check is given the kernels' own
  if (const int err = kgs::attn::check_fwd(a, lse, false, HD, HD, 0)) return err;
  const long nwg = (long)B * H * (S / QB);
  if (lse)
    hipLaunchKernelGGL(fwd<true>, dim3((unsigned)nwg), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(fwd<false>, dim3((unsigned)nwg), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// dq/dk/dv of the attention above from o, dout and lse. ws: fp32 [B*H*S]
// workspace (delta). stages: bit 0 bwd_prep, bit 1 bwd_dkdv, bit 2 bwd_dq (the
// benchmark times them apart; kgs_attn64_bwd_bf16 runs all three). Allocates
// nothing and synchronises nothing.
KGS_EXPORT int kgs_attn64_bwd_bf16_ex(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                     const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H,
                                     int HKV, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq, long lddk,
                                     long lddv, float scale, int causal, int stages, hipStream_t s) {
  using namespace kgs::attn64;
  const BwdArgs a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v,
                  (const unsigned short*)o, (const unsigned short*)dout, (const float*)lse, (float*)ws,
                  (unsigned short*)dq, (unsigned short*)dk, (unsigned short*)dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk,
                  lddv, B, S, H, HKV, scale, scale * LOG2E, causal ? 1 : 0};
  // no head_dim argument here either
  if (const int err = kgs::attn::check_bwd(a, HD, HD, 0)) return err;
  return kgs::attn::launch_bwd(bwd_prep, bwd_dkdv, bwd_dq, a, HD, KB, stages, s);
}

KGS_EXPORT int kgs_attn64_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                  const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H,
                                  int HKV, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq, long lddk,
                                  long lddv, float scale, int causal, hipStream_t s) {
  return kgs_attn64_bwd_bf16_ex(q, k, v, o, dout, lse, dq, dk, dv, ws, B, S, H, HKV, ldq, ldk, ldv, ldo, lddo, lddq,
                                lddk, lddv, scale, causal, 7, s);
}
