// Flash-attention for training on gfx950: the forward that also stores each
// query row's log-sum-exp, and the backward (dQ, dK, dV) that recomputes P from
// it. bf16 in/out, fp32 softmax/accumulate, head_dim 128, causal or full, GQA,
// Sk == S. All operands are token-major with any row stride, so q/k/v and
// dq/dk/dv can be the three column groups of a fused QKV / dQKV buffer.
//
//   P = exp2(c S - lse log2 e), c = scale log2 e     delta = rowsum(dO o O)
//   dV = P^T dO     dP = dO V^T     dS = scale P o (dP - delta)
//   dQ = dS K       dK = dS^T Q
//
// P and dS are rounded to bf16 once, as MFMA operands; everything else is fp32.
//
// Three launches, none of which waits on another workgroup and none of which
// uses an atomic: every sum has a fixed order, so the results are bitwise
// reproducible. The price is that S and dP are computed twice (14 MFMA
// products per tile pair instead of 10).
//
//   * bwd_prep: delta[b H + h, s] (fp32), memory bound.
//   * bwd_dkdv: one workgroup = 4 waves x 32 keys of one (batch, KV head); a
//     wave keeps its keys' K and V fragments and the dK^T / dV^T accumulators
//     in registers (one wave per SIMD) while the workgroup sweeps the group's
//     query heads x 64-row query tiles, so dK and dV of a KV head are summed
//     over its query heads inside the workgroup. The KEY is on the MFMA lane
//     (S = Q K^T, dP = dO V^T): the P and dS accumulators are the B operands of
//     dV^T += dO^T P and dK^T += Q^T dS with no data movement. Q and dO tiles
//     arrive by LDS-DMA in the forward's XOR image (attention_fwd.h), read by
//     rows for S / dP and by ds_read_b64_tr_b16 for the transposed operands;
//     the tile's lse and delta ride in the same DMA. A lone wave per SIMD
//     cannot hide a drained DMA, so the transposed reads are inline asm behind
//     the loop's own vmcnt + barrier and nothing inside a tile waits on vector
//     memory (docs/architecture.md, "LDS-DMA alias waits").
//     Causal: only query tiles at or after the key block are swept, waves
//     skip tiles wholly before their keys, heaviest key blocks dispatch first.
//   * bwd_dq: the mirror of the forward. One workgroup = 4 waves x 32 query
//     rows of one (q-block, head), a lane owns one query row (lse and delta
//     are lane scalars), S^T = K Q^T and dP^T = V dO^T with the Q and dO
//     fragments in registers, dQ^T += K^T dS^T with dS^T straight from the
//     accumulator and K^T by transposed reads. K/V double buffer by LDS-DMA,
//     causal tiles skipped per wave, exactly as in the forward.
#include "attention_fwd.h"

namespace kgs {
namespace attn_train {

using attn::Args;
using attn::f32x16;
using attn::HD;
using attn::KB;
using attn::off;
using attn::pack8;
using attn::QB;
using attn::swz;
using attn::TILE_BYTES;
using attn::tr_frag;

constexpr float LOG2E = 1.4426950408889634f;

struct LseArgs {
  Args a;
  float* lse;  // fp32 [B*H, S], natural log
};

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void fwd_lse(LseArgs p) {
  using namespace attn;
  constexpr bool LSE = true;
  const Args a = p.a;
  float* const lse = p.lse;
#include "attention_fwd_body.h"
}

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
  int causal;
};

// delta[b H + h, s] = sum_d dO[b s, h, d] O[b s, h, d]: 16 lanes x 8 elements
// per (token, head), summed in-lane and then by a fixed xor tree.
__global__ __launch_bounds__(256) void bwd_prep(BwdArgs a) {
  const long item = (long)blockIdx.x * 16 + (threadIdx.x >> 4);  // (token, head)
  const long total = (long)a.B * a.S * a.H;
  const int part = threadIdx.x & 15;
  float acc = 0.f;
  long tok = 0;
  int h = 0;
  if (item < total) {
    tok = item / a.H;
    h = (int)(item - tok * a.H);
    const uint4 x = *(const uint4*)(a.o + tok * a.ldo + (long)h * HD + 8 * part);
    const uint4 y = *(const uint4*)(a.dout + tok * a.lddo + (long)h * HD + 8 * part);
    const unsigned xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc = __builtin_fmaf(bf2f((unsigned short)(xs[i] & 0xffff)), bf2f((unsigned short)(ys[i] & 0xffff)), acc);
      acc = __builtin_fmaf(bf2f((unsigned short)(xs[i] >> 16)), bf2f((unsigned short)(ys[i] >> 16)), acc);
    }
  }
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 16);
  if (item < total && part == 0) {
    const long b = tok / a.S, srow = tok - b * a.S;
    a.delta[(b * a.H + h) * a.S + srow] = acc;
  }
}

// acc (rows (r&3) + 8 (r>>2) + 4 hh of a 32-row block on the registers, the
// lane's column on l32) -> 32 bf16 columns 32 d + ... of the lane's row.
__device__ __forceinline__ void store_acc_row(unsigned short* rowp, const f32x16 (&acc)[4], int hh) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      uint2 pk;
      pk.x = pack_bf16x2(acc[d][4 * r4 + 0], acc[d][4 * r4 + 1]);
      pk.y = pack_bf16x2(acc[d][4 * r4 + 2], acc[d][4 * r4 + 3]);
      *(uint2*)(rowp + 32 * d + 8 * r4 + 4 * hh) = pk;
    }
}

// X^T fragments (A operand) of rows rb .. rb+15 x columns 32 d + l32 of a tile
// in the XOR image, in the k order of an accumulator used as the B operand
// (attention_fwd.h: row = rb + 8 (e>>2) + 4 hh + (e&3) for element e).
__device__ __forceinline__ bf16x8 tr_rows(const char* tile, int rb, int d, int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3, hh = lane >> 5;
  const int c0 = 4 * d + 2 * (g & 1) + (tp >> 1);
  const int row = rb + 4 * hh + tq;
  return tr_frag(tile + off(row, c0) + 8 * (tp & 1), tile + off(row + 8, c0) + 8 * (tp & 1));
}

// The same fragment by inline-asm reads, for a loop that keeps an LDS-DMA in
// flight: hipcc puts a vmcnt(0) before a BUILTIN ds_read_tr then (its LDS-DMA
// alias check), which drains the DMA. The caller orders the DMA before these
// reads (its own vmcnt + barrier) and retires them with tr_wait before use.
struct TrPair {
  attn::bf16x4s lo, hi;
};
__device__ __forceinline__ TrPair tr_rows_asm(const char* tile, int rb, int d, int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3, hh = lane >> 5;
  const int c0 = 4 * d + 2 * (g & 1) + (tp >> 1);
  const int row = rb + 4 * hh + tq;
  const unsigned a0 = (unsigned)(uintptr_t)(const KGS_LDS char*)(tile + off(row, c0) + 8 * (tp & 1));
  const unsigned a1 = (unsigned)(uintptr_t)(const KGS_LDS char*)(tile + off(row + 8, c0) + 8 * (tp & 1));
  TrPair r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r.lo) : "v"(a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r.hi) : "v"(a1));
  return r;
}
// lgkmcnt(0) tied to the eight fragments read above: every use of them depends
// on this statement, so no consumer can be scheduled ahead of the wait
__device__ __forceinline__ void tr_wait(TrPair (&f)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi), "+v"(f[2].lo), "+v"(f[2].hi),
                 "+v"(f[3].lo), "+v"(f[3].hi), "+v"(f[4].lo), "+v"(f[4].hi), "+v"(f[5].lo), "+v"(f[5].hi),
                 "+v"(f[6].lo), "+v"(f[6].hi), "+v"(f[7].lo), "+v"(f[7].hi));
}
__device__ __forceinline__ bf16x8 tr_join(const TrPair& f) {
  return __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

constexpr int KBW = 128;  // keys per bwd_dkdv workgroup (4 waves x 32)

__global__ __launch_bounds__(256, 1) void bwd_dkdv(BwdArgs a) {
  // [buf][Q | dO (64 query rows each) | their lse | their delta | pad]
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
  const int k0 = kbi * KBW;
  const int kw = k0 + 32 * w;   // this wave's first key
  const int key = kw + l32;     // this lane's key
  const long tok0 = (long)b * a.S;

  // K and V fragments (B operands of S = Q.K^T and dP = dO.V^T): lane holds
  // K[key][16 ks + 8 hh .. +7]
  bf16x8 kf[8], vf[8];
  {
    const bf16x8* kp = (const bf16x8*)(a.k + (tok0 + key) * a.ldk + (long)kvh * HD + 8 * hh);
    const bf16x8* vp = (const bf16x8*)(a.v + (tok0 + key) * a.ldv + (long)kvh * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      kf[ks] = kp[2 * ks];
      vf[ks] = vp[2 * ks];
    }
  }

  const int nqt = a.S / KB;                     // 64-row query tiles per head
  const int qt0 = a.causal ? k0 / KB : 0;       // first tile that sees this key block
  const int nper = nqt - qt0;
  const int niter = G * nper;

  // Q / dO tile of iteration it -> LDS buffer sb, the forward's chunking: wave
  // w issues chunks 4w .. 4w+3 (4 rows of 256 B each) of Q and of dO.
  auto dma_tiles = [&](int it, int sb) {
    const int hg = it / nper, qt = qt0 + (it - hg * nper);
    const int h = kvh * G + hg;
    const unsigned short* qbase = a.q + (tok0 + (long)qt * KB) * a.ldq + (long)h * HD;
    const unsigned short* dobase = a.dout + (tok0 + (long)qt * KB) * a.lddo + (long)h * HD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 4 * w + i;
      const int r = 4 * ch + (lane >> 4), c = (lane & 15) ^ swz(r);
      glds16(qbase + (long)r * a.ldq + 8 * c, smem[sb] + 1024 * ch);
      glds16(dobase + (long)r * a.lddo + 8 * c, smem[sb] + TILE_BYTES + 1024 * ch);
    }
    // the tile's 64 lse and 64 delta values (256 B each) ride along: lanes
    // 0-15 fetch lse, 16-31 delta, 32-63 the same again into the pad
    if (w == 0) {
      const long rowoff = ((long)b * a.H + h) * a.S + (long)qt * KB;
      const float* src = ((lane & 16) ? a.delta : a.lse) + rowoff + 4 * (lane & 15);
      glds16(src, smem[sb] + ROWS_OFF);
    }
  };

  dma_tiles(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): K/V fragments and tile 0
  __syncthreads();

  f32x16 dk[4], dv[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    dk[d] = f32x16{};
    dv[d] = f32x16{};
  }
  const float sl2 = a.sl2, scale = a.scale;

  for (int it = 0; it < niter; ++it) {
    const int buf = it & 1;
    const int hg = it / nper, qt = qt0 + (it - hg * nper);
    const int h = kvh * G + hg;
    const int q0 = qt * KB;
    // the other buffer was released by the previous iteration's barrier
    if (it + 1 < niter) dma_tiles(it + 1, buf ^ 1);
    if (!a.causal || q0 + KB - 1 >= kw) {
      const char* Qs = smem[buf];
      const char* Ds = smem[buf] + TILE_BYTES;
      const char* Ls = smem[buf] + ROWS_OFF;
      f32x16 s[2], dp[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = f32x16{};
        dp[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const bf16x8 qa = *(const bf16x8*)(Qs + off(32 * t + l32, 2 * ks + hh));
          s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s[t], 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const bf16x8 da = *(const bf16x8*)(Ds + off(32 * t + l32, 2 * ks + hh));
          dp[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], dp[t], 0, 0, 0);
        }
      }
      const bool diag = a.causal && q0 < kw + 31;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          // register 4 r4 + i is query row 32 t + 8 r4 + 4 hh + i of the tile
          const int qr = 32 * t + 8 * r4 + 4 * hh;
          const f32x4 ls = *(const f32x4*)(Ls + 4 * qr);
          const f32x4 de = *(const f32x4*)(Ls + 256 + 4 * qr);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * r4 + i;
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -ls[i] * LOG2E));
            if (diag && key > q0 + qr + i) p = 0.f;
            s[t][r] = p;
            dp[t][r] = scale * (p * (dp[t][r] - de[i]));
          }
        }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const bf16x8 pf = pack8(s[t], 8 * sp), dsf = pack8(dp[t], 8 * sp);
          TrPair f[8];  // dO^T (0-3) and Q^T (4-7) of these 16 query rows
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            f[d] = tr_rows_asm(Ds, 32 * t + 16 * sp, d, lane);
            f[4 + d] = tr_rows_asm(Qs, 32 * t + 16 * sp, d, lane);
          }
          tr_wait(f);
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_join(f[d]), pf, dv[d], 0, 0, 0);
            dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_join(f[4 + d]), dsf, dk[d], 0, 0, 0);
          }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }

  store_acc_row(a.dk + (tok0 + key) * a.lddk + (long)kvh * HD, dk, hh);
  store_acc_row(a.dv + (tok0 + key) * a.lddv + (long)kvh * HD, dv, hh);
}

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void bwd_dq(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2][2][TILE_BYTES];  // [buf][K, V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int nqb = a.S / QB;
  const int nwg = gridDim.x;
  // the forward's dispatch order (heaviest q-blocks first, a KV group's heads
  // on one XCD back to back)
  int lid = blockIdx.x;
  if ((nwg & 31) == 0) {
    const int t = lid >> 3, x = lid & 7;
    lid = ((t >> 2) << 5) | (x << 2) | (t & 3);
  }
  const int per = a.B * a.H;
  const int qi = lid / per, rem = lid - qi * per;
  const int qb = a.causal ? nqb - 1 - qi : qi;
  const int b = rem / a.H, h = rem - b * a.H;
  const int kvh = h / (a.H / a.HKV);

  const int q0 = qb * QB;
  const int qw = q0 + 32 * w;   // this wave's first query row
  const int qrow = qw + l32;    // this lane's query row
  const long tok0 = (long)b * a.S;

  // Q and dO fragments (B operands of S^T = K.Q^T and dP^T = V.dO^T)
  bf16x8 qf[8], dof[8];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (tok0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
    const bf16x8* dp_ = (const bf16x8*)(a.dout + (tok0 + qrow) * a.lddo + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 4 * w + i;
      const int r = 4 * ch + (lane >> 4), c = (lane & 15) ^ swz(r);
      const long row = (long)jn * KB + r;
      glds16(kbase + row * a.ldk + 8 * c, smem[sb][0] + 1024 * ch);
      glds16(vbase + row * a.ldv + 8 * c, smem[sb][1] + 1024 * ch);
    }
  };

  const int ntile = a.causal ? (q0 + QB) / KB : a.S / KB;
  dma_tiles(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the fragments, lse, delta and tile 0
  __syncthreads();

  f32x16 dq[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) dq[d] = f32x16{};
  const float sl2 = a.sl2, scale = a.scale;

  for (int j = 0; j < ntile; ++j) {
    const int buf = j & 1;
    if (j + 1 < ntile) dma_tiles(j + 1, buf ^ 1);
    const int kv0 = j * KB;
    if (!a.causal || kv0 <= qw + 31) {
      const char* Ks = smem[buf][0];
      const char* Vs = smem[buf][1];
      f32x16 s[2], dp[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = f32x16{};
        dp[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const bf16x8 ka = *(const bf16x8*)(Ks + off(32 * t + l32, 2 * ks + hh));
          s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[ks], s[t], 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const bf16x8 va = *(const bf16x8*)(Vs + off(32 * t + l32, 2 * ks + hh));
          dp[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, dof[ks], dp[t], 0, 0, 0);
        }
      }
      const bool diag = a.causal && kv0 + KB - 1 > qw;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -lse2));
          if (diag && kv > qrow) p = 0.f;
          dp[t][r] = scale * (p * (dp[t][r] - delta));
        }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const bf16x8 dsf = pack8(dp[t], 8 * sp);
#pragma unroll
          for (int d = 0; d < 4; ++d)
            dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_rows(Ks, 32 * t + 16 * sp, d, lane), dsf, dq[d], 0, 0, 0);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }

  store_acc_row(a.dq + (tok0 + qrow) * a.lddq + (long)h * HD, dq, hh);
}

}  // namespace attn_train
}  // namespace kgs

// The forward of kgs_attn_fwd_bf16 (same requirements, same output bits) that
// also writes lse[b H + h, s] = ln sum_k exp(scale q.k), fp32 [B*H, S].
KGS_EXPORT int kgs_attn_fwd_lse_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int S,
                                    int H, int HKV, int hd, long ldq, long ldk, long ldv, long ldo, float scale,
                                    int causal, hipStream_t s) {
  using namespace kgs::attn;
  if (B <= 0 || S <= 0 || H <= 0 || HKV <= 0 || H % HKV) return KGS_ERR_SHAPE;
  if (hd != HD || S % QB) return KGS_ERR_SHAPE;
  if (ldq < (long)H * HD || ldk < (long)HKV * HD || ldv < (long)HKV * HD || ldo < (long)H * HD) return KGS_ERR_SHAPE;
  const uintptr_t al = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)lse;
  if (!lse || (al & 15) || (ldq | ldk | ldv | ldo) & 7) return KGS_ERR_ALIGN;
  const long nwg = (long)B * H * (S / QB);
  if (nwg > 0x7fffffff) return KGS_ERR_SHAPE;
  kgs::attn_train::LseArgs p{{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v,
                              (unsigned short*)o, ldq, ldk, ldv, ldo, B, S, H, HKV,
                              scale * 1.4426950408889634f, causal ? 1 : 0, S, 0},
                             (float*)lse};
  hipLaunchKernelGGL(kgs::attn_train::fwd_lse, dim3((unsigned)nwg), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

// dq/dk/dv of the attention above from o, dout and lse. ws: fp32 [B*H*S]
// workspace (delta). stages: bit 0 bwd_prep, bit 1 bwd_dkdv, bit 2 bwd_dq (the
// benchmark times them apart; kgs_attn_bwd_bf16 runs all three). Allocates
// nothing and synchronises nothing.
KGS_EXPORT int kgs_attn_bwd_bf16_ex(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                   const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H,
                                   int HKV, int hd, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq,
                                   long lddk, long lddv, float scale, int causal, int stages, hipStream_t s) {
  using namespace kgs::attn;
  using namespace kgs::attn_train;
  if (B <= 0 || S <= 0 || H <= 0 || HKV <= 0 || H % HKV) return KGS_ERR_SHAPE;
  if (hd != HD || S % QB) return KGS_ERR_SHAPE;
  const long qc = (long)H * HD, kc = (long)HKV * HD;
  if (ldq < qc || ldo < qc || lddo < qc || lddq < qc || ldk < kc || ldv < kc || lddk < kc || lddv < kc)
    return KGS_ERR_SHAPE;
  if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv || !ws) return KGS_ERR_ALIGN;
  const uintptr_t al = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dout | (uintptr_t)lse |
                       (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)ws;
  if ((al & 15) || (ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv) & 7) return KGS_ERR_ALIGN;
  const long items = (long)B * S * H;
  const long nprep = (items + 15) / 16, ndq = (long)B * H * (S / QB), nkv = (long)B * HKV * (S / KBW);
  if (nprep > 0x7fffffff) return KGS_ERR_SHAPE;
  BwdArgs a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (const unsigned short*)o,
            (const unsigned short*)dout, (const float*)lse, (float*)ws, (unsigned short*)dq, (unsigned short*)dk,
            (unsigned short*)dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, B, S, H, HKV, scale,
            scale * LOG2E, causal ? 1 : 0};
  if (stages & 1) hipLaunchKernelGGL(bwd_prep, dim3((unsigned)nprep), dim3(256), 0, s, a);
  if (stages & 2) hipLaunchKernelGGL(bwd_dkdv, dim3((unsigned)nkv), dim3(256), 0, s, a);
  if (stages & 4) hipLaunchKernelGGL(bwd_dq, dim3((unsigned)ndq), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

KGS_EXPORT int kgs_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H, int HKV,
                                int hd, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq, long lddk,
                                long lddv, float scale, int causal, hipStream_t s) {
  return kgs_attn_bwd_bf16_ex(q, k, v, o, dout, lse, dq, dk, dv, ws, B, S, H, HKV, hd, ldq, ldk, ldv, ldo, lddo, lddq,
                              lddk, lddv, scale, causal, 7, s);
}
