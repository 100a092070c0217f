// Sliding-window causal flash attention for training on gfx950: forward (with
// or without the log-sum-exp) and backward (delta, dK/dV, dQ). Query row i of a
// sequence sees the W keys max(0, i - W + 1) .. i (HF sliding_window = W,
// flash-attn window_size = (W - 1, 0)). The contract is attention_train.hip's:
// head_dim 128, bf16 in/out, fp32 softmax and accumulation, GQA, S % 128 == 0,
// token-major operands with any row stride (column groups of a fused QKV / dQKV
// buffer). The math is that file's too; what differs is which tiles are walked,
// in which order, and where the mask code sits.
//
// The MFMA scheme is the project's: a lane owns a query row (a key in dK/dV),
// the swapped product S^T = K Q^T on v_mfma_f32_32x32x16_bf16 leaves the row's
// scores in the lane's registers, softmax is in-lane, the P / dS accumulator is
// the next product's B operand as it stands, tiles arrive by LDS-DMA in the XOR
// image of attention_fwd.h into a double buffer, and transposed operands come
// from ds_read_b64_tr_b16.
//
// Tile range, bounded on both sides. One predicate masks both edges: entry
// (i, j) is visible iff 0 <= i - j < W, i.e. unsigned(i - j) < unsigned(W).
//   * fwd, bwd_dq: a 128-row q-block at q0 walks the 64-key tiles that meet
//     [q0 - W + 1, q0 + 127]; a wave (32 rows from qw) computes a tile only if
//     it meets [qw - W + 1, qw + 31], and runs the mask code only if the tile
//     has a key above qw (causal edge) or a key W or more below qw + 31 (window
//     edge). For W < 96 both edges fall into one tile; interior tiles carry no
//     mask code.
//   * bwd_dkdv: a 128-key block at k0 sweeps, per query head of its KV group,
//     the 64-row query tiles that meet [k0, min(S, k0 + 127 + W) - 1]; a wave
//     (32 keys from kw) computes a tile only if it meets [kw, kw + 30 + W].
//   Work per workgroup is O(W), whatever S is: at most W / 64 + 3 tiles in fwd
//   and bwd_dq, and that many per query head of the KV group in bwd_dkdv
//   (G (W / 64 + 3) for a group of G heads).
//
// The empty-first-tile hazard. Under the plain causal mask every row sees key
// 0, so the first tile walked gives every row a finite running max. Under a
// window the LOWEST tile a wave walks can be wholly masked for some of its rows
// (whenever W is not a multiple of 64, or the row is not the wave's first):
// with the max still at the -1e30 sentinel, exp2(s - m) of a masked score is
// exp2(0) = 1, which poisons the row sum and O, and the deferred rescale would
// carry it along. The forward therefore walks key tiles DOWNWARD from the
// diagonal. A wave's rows qw .. qw + 31 are 32-aligned, so the first tile it
// computes (the 64-key tile holding qw + 31) holds every row's own key: after
// it every running max is a real score, and a masked score (-1e30) in any
// later tile gives exp2(-1e30 sl2 - m sl2) = 0 exactly. The backward does not
// depend on the order (P comes from lse) and selects masked P to 0.0f after
// the exp2, so masked entries of P and dS are exact zeros.
//
// Dispatch: past the first W / 128 blocks every q-block and every key block
// costs the same, so blocks go out in ascending order (no heaviest-first
// reversal); the XCD grouping that puts the heads of one KV group back to back
// on one XCD is kept. fwd and bwd_dq run two workgroups per CU (64 KB LDS, 256
// registers), bwd_dkdv one wave per SIMD with its K, V, dK^T and dV^T resident.
// No atomics, no cross-workgroup waits, no memset: every sum has a fixed order
// and the launches can be captured in a graph. The only workspace is the fp32
// delta [B*H, S].
#include "attention_train.h"

namespace kgs {
namespace attn_win {

using attn::BwdArgs;
using attn::dispatch_id;
using attn::dma_pair;
using attn::f32x16;
using attn::FwdArgs;
using attn::HD;
using attn::KB;
using attn::KBW;
using attn::LOG2E;
using attn::NEG;
using attn::off;
using attn::pack8;
using attn::QB;
using attn::RESCALE;
using attn::store_acc_row;
using attn::swz;
using attn::TILE_BYTES;
using attn::tr_frag;
using attn::tr_join;
using attn::tr_rows;
using attn::tr_rows_asm;
using attn::tr_wait;
using attn::TrPair;

// (query i, key j) is outside the window or above the diagonal
__device__ __forceinline__ bool hidden(int i, int j, int W) { return (unsigned)(i - j) >= (unsigned)W; }

template <bool LSE>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void fwd(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2][2 * TILE_BYTES];  // [buf][K | V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int lid = dispatch_id(blockIdx.x, gridDim.x);
  const int per = a.B * a.H;
  const int qb = lid / per, rem = lid - qb * per;
  const int b = rem / a.H, h = rem - b * a.H;
  const int kvh = h / (a.H / a.HKV);
  const int W = a.mask;

  const int q0 = qb * QB;
  const int qw = q0 + 32 * w;  // this wave's first query row
  const int qrow = qw + l32;   // this lane's query row
  const long tok0 = (long)b * a.S;

  // Q fragments (B operand of S^T = K.Q^T): lane holds Q[qrow][16ks + 8hh .. +7]
  bf16x8 qf[8];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (tok0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = qp[2 * ks];
  }
  const unsigned short* kbase = a.k + tok0 * a.ldk + (long)kvh * HD;
  const unsigned short* vbase = a.v + tok0 * a.ldv + (long)kvh * HD;

  // key tiles jhi, jhi - 1, .., jlo: downward from the diagonal (file header)
  const int jhi = (q0 + QB - 1) / KB;
  const int jlo = (q0 - W + 1 > 0 ? q0 - W + 1 : 0) / KB;
  const int ntile = jhi - jlo + 1;
  dma_pair(kbase, vbase, a.ldk, a.ldv, jhi, smem[0], w, lane);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): Q fragments and the first tile
  __syncthreads();

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = f32x16{};
  float m = NEG, l = 0.f;
  const float sl2 = a.sl2;
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;  // tr-read address pieces

  for (int j = 0; j < ntile; ++j) {
    const int buf = j & 1;
    // the other buffer was released by the previous tile's barrier
    if (j + 1 < ntile) dma_pair(kbase, vbase, a.ldk, a.ldv, jhi - j - 1, smem[buf ^ 1], w, lane);
    const int kv0 = (jhi - j) * KB;
    // the tile meets [qw - W + 1, qw + 31]
    if (kv0 <= qw + 31 && kv0 + KB - 1 + W > qw) {
      const char* Ks = smem[buf];
      const char* Vs = smem[buf] + TILE_BYTES;
      bf16x8 kf[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[t][ks] = *(const bf16x8*)(Ks + off(32 * t + l32, 2 * ks + hh));
      __builtin_amdgcn_sched_barrier(0);  // all K reads ahead of the MFMAs
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[t][ks], qf[ks], s[t], 0, 0, 0);
      }
      // a quarter of the V fragments now (their latency hides under the softmax),
      // the rest under the first P.V MFMAs: with the two-edge mask in between,
      // half of them ahead (as the causal forward reads) spills at 2 waves per SIMD
      bf16x8 vfr[4][2][2];
      auto read_v = [&](int d) {
        const int c0 = 4 * d + 2 * (g & 1) + (tp >> 1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int sp = 0; sp < 2; ++sp) {
            const int kvb = 32 * t + 16 * sp + 4 * hh + tq;
            vfr[d][t][sp] = tr_frag(Vs + off(kvb, c0) + 8 * (tp & 1), Vs + off(kvb + 8, c0) + 8 * (tp & 1));
          }
      };
      read_v(0);
      __builtin_amdgcn_sched_barrier(0);
      // causal edge: a key above the wave's first row; window edge: a key W or
      // more below its last row
      if (kv0 + KB - 1 > qw || qw + 31 - kv0 >= W) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (hidden(qrow, kv, W)) s[t][r] = NEG;
          }
      }
      float mx = m;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
      mx = xor32_max(mx);
      // deferred rescale: m moves only when a row's new max exceeds it by more
      // than RESCALE (log2 units), so p <= 2^RESCALE; wave-uniform decision.
      // The first computed tile always moves it off the sentinel (alpha = 0).
      const bool grow = (mx - m) * sl2 > RESCALE;
      if (__any(grow)) {
        const float mn = grow ? mx : m;
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sl2);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] *= alpha;
      }
      const float msl = m * sl2;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -msl));
          s[t][r] = p;
          l += p;
        }
      bf16x8 pf[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        pf[t][0] = pack8(s[t], 0);
        pf[t][1] = pack8(s[t], 8);
      }
      read_v(1);
      read_v(2);
      read_v(3);
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int sp = 0; sp < 2; ++sp)
            o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[d][t][sp], pf[t][sp], o[d], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the next tile has landed
    __syncthreads();
  }

  l = xor32_sum(l);
  if constexpr (LSE) {
    // ln sum exp(scale s) = (m sl2 + log2 l) ln 2
    if (hh == 0)
      a.lse[((long)b * a.H + h) * a.S + qrow] = (m * sl2 + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
  }
  const float inv = 1.0f / l;
  store_acc_row(a.o + (tok0 + qrow) * a.ldo + (long)h * HD, o, hh, inv);
}

__global__ __launch_bounds__(256) void bwd_prep(BwdArgs a) { attn::prep_body<HD>(a); }

__global__ __launch_bounds__(256, 1) void bwd_dkdv(BwdArgs a) {
  // [buf][Q | dO (64 query rows each) | their lse | their delta | pad]
  constexpr int ROWS_OFF = 2 * TILE_BYTES, BUF_BYTES = ROWS_OFF + 1024;
  __shared__ __attribute__((aligned(16))) char smem[2][BUF_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int G = a.H / a.HKV;
  const int W = a.mask;
  // ascending key blocks: the last W / 128 blocks, whose sweep S clips, go last
  const int per = a.B * a.HKV;
  const int kbi = blockIdx.x / per, rem = blockIdx.x - kbi * per;
  const int b = rem / a.HKV, kvh = rem - b * a.HKV;
  const int k0 = kbi * KBW;
  const int kw = k0 + 32 * w;  // this wave's first key
  const int key = kw + l32;    // this lane's key
  const long tok0 = (long)b * a.S;

  // K and V fragments (B operands of S = Q.K^T and dP = dO.V^T)
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

  // 64-row query tiles qt0 .. qt0 + nper - 1 meet the rows that see this key
  // block, [k0, min(S, k0 + 127 + W) - 1]; the sweep repeats per query head
  const int qt0 = k0 / KB;
  const int rend = k0 + KBW - 1 + W < a.S ? k0 + KBW - 1 + W : a.S;  // one past the last such row
  const int nper = (rend + KB - 1) / KB - qt0;
  const int niter = G * nper;

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
    const int q0 = qt * KB;
    // the other buffer was released by the previous iteration's barrier
    if (it + 1 < niter) dma_tiles(it + 1, buf ^ 1);
    // the tile meets the rows that see this wave's keys, [kw, kw + 30 + W]
    if (q0 + KB - 1 >= kw && q0 - kw - 31 < W) {
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
      // causal edge: a row below the wave's last key; window edge: a row W or
      // more above its first key
      const bool edge = q0 < kw + 31 || q0 + KB - 1 - kw >= W;
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
            if (edge && hidden(q0 + qr + i, key, W)) p = 0.f;
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
  __shared__ __attribute__((aligned(16))) char smem[2][2 * TILE_BYTES];  // [buf][K | V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int lid = dispatch_id(blockIdx.x, gridDim.x);
  const int per = a.B * a.H;
  const int qb = lid / per, rem = lid - qb * per;
  const int b = rem / a.H, h = rem - b * a.H;
  const int kvh = h / (a.H / a.HKV);
  const int W = a.mask;

  const int q0 = qb * QB;
  const int qw = q0 + 32 * w;  // this wave's first query row
  const int qrow = qw + l32;   // this lane's query row
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

  // the forward's tiles in the forward's order
  const int jhi = (q0 + QB - 1) / KB;
  const int jlo = (q0 - W + 1 > 0 ? q0 - W + 1 : 0) / KB;
  const int ntile = jhi - jlo + 1;
  dma_pair(kbase, vbase, a.ldk, a.ldv, jhi, smem[0], w, lane);
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the fragments, lse, delta and the first tile
  __syncthreads();

  f32x16 dq[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) dq[d] = f32x16{};
  const float sl2 = a.sl2, scale = a.scale;

  for (int j = 0; j < ntile; ++j) {
    const int buf = j & 1;
    if (j + 1 < ntile) dma_pair(kbase, vbase, a.ldk, a.ldv, jhi - j - 1, smem[buf ^ 1], w, lane);
    const int kv0 = (jhi - j) * KB;
    if (kv0 <= qw + 31 && kv0 + KB - 1 + W > qw) {
      const char* Ks = smem[buf];
      const char* Vs = smem[buf] + TILE_BYTES;
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
      const bool edge = kv0 + KB - 1 > qw || qw + 31 - kv0 >= W;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sl2, -lse2));
          if (edge && hidden(qrow, kv, W)) p = 0.f;
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

}  // namespace attn_win
}  // namespace kgs

// Sliding-window causal attention forward: kgs_attn_fwd_lse_bf16's arguments
// plus `window` (row i sees keys max(0, i - window + 1) .. i; window >= S is
// plain causal). lse (fp32 [B*H, S], natural log) may be null: the output bits
// are the same. window < 1 is KGS_ERR_SHAPE, causal == 0 is KGS_ERR_ARG; a bad
// argument launches nothing.
KGS_EXPORT int kgs_attn_win_fwd_bf16(const void* q, const void* k, const void* v, void* o, void* lse, int B, int S,
                                    int H, int HKV, int hd, long ldq, long ldk, long ldv, long ldo, float scale,
                                    int causal, int window, hipStream_t s) {
  using namespace kgs::attn;
  using namespace kgs::attn_win;
  const FwdArgs p{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)o,
                  (float*)lse, ldq, ldk, ldv, ldo, B, S, H, HKV, scale * LOG2E, window < S ? window : S};
  if (const int err = check_fwd(p, lse, false, hd, HD, window < 1 ? KGS_ERR_SHAPE : !causal ? KGS_ERR_ARG : 0))
    return err;
  const long nwg = (long)B * H * (S / QB);
  if (lse)
    hipLaunchKernelGGL(fwd<true>, dim3((unsigned)nwg), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(fwd<false>, dim3((unsigned)nwg), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

// dq/dk/dv of the attention above from o, dout and lse: kgs_attn_bwd_bf16_ex's
// arguments plus `window`. ws: fp32 [B*H*S] workspace (delta). stages: bit 0
// bwd_prep, bit 1 bwd_dkdv, bit 2 bwd_dq. Allocates and synchronises nothing.
KGS_EXPORT int kgs_attn_win_bwd_bf16_ex(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                       const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H,
                                       int HKV, int hd, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq,
                                       long lddk, long lddv, float scale, int causal, int window, int stages,
                                       hipStream_t s) {
  using namespace kgs::attn;
  using namespace kgs::attn_win;
  const BwdArgs a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v,
                  (const unsigned short*)o, (const unsigned short*)dout, (const float*)lse, (float*)ws,
                  (unsigned short*)dq, (unsigned short*)dk, (unsigned short*)dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk,
                  lddv, B, S, H, HKV, scale, scale * LOG2E, window < S ? window : S};
  if (const int err = check_bwd(a, hd, HD, window < 1 ? KGS_ERR_SHAPE : !causal ? KGS_ERR_ARG : 0)) return err;
  return launch_bwd(bwd_prep, bwd_dkdv, bwd_dq, a, HD, KBW, stages, s);
}

KGS_EXPORT int kgs_attn_win_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                    const void* lse, void* dq, void* dk, void* dv, void* ws, int B, int S, int H,
                                    int HKV, int hd, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq,
                                    long lddk, long lddv, float scale, int causal, int window, hipStream_t s) {
  return kgs_attn_win_bwd_bf16_ex(q, k, v, o, dout, lse, dq, dk, dv, ws, B, S, H, HKV, hd, ldq, ldk, ldv, ldo, lddo,
                                  lddq, lddk, lddv, scale, causal, window, 7, s);
}
