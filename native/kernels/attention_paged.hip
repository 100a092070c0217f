// Paged prefill attention for gfx950: causal flash-attention forward (bf16 in /
// out, fp32 softmax / accumulate, head_dim 128, GQA) of prompt CHUNKS over the
// paged bf16 KV cache, read in place. One launch serves every prompt chunk of a
// chunked-prefill step -- first chunks of any length, continuation chunks and
// prefix-cache hits -- with no gather of the cached context into row-major K / V
// (kgs.ops.decode.gather_kv + attention.hip's fwd is the path this replaces).
//
// Inputs: Q rows of the fused, rotated QKV buffer; one layer of the cache
// ([pages, HKV, 2, 4096] bf16, 32-token pages in decode.hip's kv_k_index /
// kv_v_index layouts); a block table [nchunks, max_pages]; per chunk a
// descriptor (row0, n, padded, ctx0): Q rows row0 .. row0+padded-1 hold positions
// ctx0 .. ctx0+padded-1, n of them real, row r < n sees keys 0 .. ctx0+r (the
// chunk's own K / V are already in the cache). padded % 128 == 0, ctx0 % 64 == 0.
//
// The kernel keeps attention.hip's shape -- one workgroup = 4 waves x 32 query
// rows of one (q-block, head), 2 workgroups per CU, swapped S^T = K . Q^T on
// v_mfma_f32_32x32x16_bf16 (a lane owns ONE query row: in-lane softmax), the
// S^T accumulator as the B operand of O^T = V^T . P^T, 64-key tiles (= 2 pages)
// in an LDS double buffer filled by LDS-DMA, deferred rescale -- and differs in
// where the fragments come from:
//   * Both regions of a page are already in 16-byte units an MFMA A operand
//     takes whole, so a page's K and V regions are copied LINEARLY into LDS
//     (every global_load_lds moves 1 KB contiguous to 1 KB contiguous, the page
//     base from the block table) and no transposed read is needed.
//   * V unit (dt, g, m) is dim 16 dt + m of tokens {4g..4g+3, 16+4g..16+4g+3}:
//     the A fragment of k-step (sp, lane half hh) with g = 2 sp + hh, PROVIDED
//     row i of a 32-row S^T tile is the page's token tau(i) = i with index bits
//     3 and 4 swapped. So lane l32 of the K read fetches token tau(l32): K unit
//     (tau, c) is dims 8c .. 8c+7 of that token, c = 2 ks + hh. The causal
//     compare runs on the true position tau, nothing else changes.
//   * LDS banks: ds_read_b128 is served in the 16-lane groups {0-3, 12-15,
//     20-27} / {4-11, 16-19, 28-31} (+32); in both linear images each group's
//     lanes land on 16 distinct 16-byte slots of the 256-byte bank row.
//   * Stale data -- block-table entries past the sequence's pages, token slots
//     at or after ctx0 + n in its last page -- is only ever seen by keys the
//     causal select masks for every real row; tiles wholly past ctx0 + n - 1
//     are not walked; rows >= n are written as zeros by select.
// The host hands over a q-block table (chunk, q-block in chunk), heaviest
// first; work id -> (q-block, head) keeps the heads of one KV group back to back
// on one XCD, as attention.hip does. No workspace, no memset, no host sync.
#include "kgs_common.h"

namespace kgs {
namespace attnp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HD = 128;
constexpr int QB = 128;                   // query rows per workgroup (4 waves x 32)
constexpr int KB = 64;                    // keys per tile = 2 pages
constexpr int PAGE = 32;                  // tokens per KV-cache page (decode.hip)
constexpr int PAGE_ELEMS = PAGE * HD;     // per (page, kv head, K|V): 8 KB
constexpr int TILE_BYTES = KB * HD * 2;   // 16 KB
constexpr float NEG = -1.0e30f;
constexpr float RESCALE = 8.0f;  // deferred-max threshold, log2 units: P <= 256

struct Args {
  const unsigned short* q;      // row 0, head 0 of the fused QKV buffer
  const unsigned short* cache;  // one layer: [pages, HKV, 2, 4096]
  const int* bt;                // [nchunks, max_pages]
  const int* desc;              // [nchunks, 4]: row0, n, padded, ctx0
  const int* qmap;              // [nqb, 2]: chunk, q-block in chunk
  unsigned short* o;
  long ldq, ldo;  // row strides (elements)
  int H, HKV, max_pages;
  float sl2;  // softmax scale * log2(e)
};

// row i of a 32-row S^T tile <-> token tau of its page: index bits 3 and 4 swapped
__device__ __forceinline__ int swap34(int i) { return (i & 7) | ((i & 8) << 1) | ((i & 16) >> 1); }

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void fwd_paged(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[2][2][TILE_BYTES];  // [buf][K, V], page t at 8 KB * t

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int nwg = gridDim.x;
  // XCD-aware order: 8 consecutive dispatch slots of one XCD take 4 heads of
  // one KV group; work ids stay heaviest-first in dispatch time.
  int lid = blockIdx.x;
  if ((nwg & 31) == 0) {
    const int t = lid >> 3, x = lid & 7;
    lid = ((t >> 2) << 5) | (x << 2) | (t & 3);
  }
  const int qi = lid / a.H, h = lid - qi * a.H;
  const int kvh = h / (a.H / a.HKV);
  const int ci = a.qmap[2 * qi], qb = a.qmap[2 * qi + 1];
  const int row0 = a.desc[4 * ci], n = a.desc[4 * ci + 1], ctx0 = a.desc[4 * ci + 3];

  const int q0 = qb * QB;
  const int qw = q0 + 32 * w;  // this wave's first query row in the chunk
  const int qrow = qw + l32;   // this lane's query row in the chunk

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = f32x16{};
  float m = NEG, l = 0.f;

  // rows >= n leave as exact zeros (a select: their accumulators may hold anything)
  auto store = [&](float inv) {
    const bool real = qrow < n;
    unsigned short* op = a.o + (long)(row0 + qrow) * a.ldo + (long)h * HD;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int dcol = 32 * d + 8 * r4 + 4 * hh;
        uint2 pk;
        pk.x = real ? pack_bf16x2(o[d][4 * r4 + 0] * inv, o[d][4 * r4 + 1] * inv) : 0u;
        pk.y = real ? pack_bf16x2(o[d][4 * r4 + 2] * inv, o[d][4 * r4 + 3] * inv) : 0u;
        *(uint2*)(op + dcol) = pk;
      }
  };
  if (q0 >= n) {  // a q-block of padding only (workgroup-uniform: before any barrier)
    store(0.f);
    return;
  }

  // Q fragments (B operand of S^T = K.Q^T): lane holds Q[qrow][16ks + 8hh .. +7]
  bf16x8 qf[8];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (long)(row0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = qp[2 * ks];
  }

  // Key tile j = pages 2j, 2j+1 of the sequence. A 16 KB K (or V) tile is 16
  // chunks of 1 KB; wave w issues chunks 4w .. 4w+3 of both, all inside page
  // w >> 1 of the tile, so a wave needs one block-table entry per tile. The
  // entry index is clamped to the table: a last tile whose second page lies
  // past an odd-width table re-reads a valid page (masked like any stale key).
  const int* bt = a.bt + (long)ci * a.max_pages;
  auto page_of = [&](int j) {
    const int pi = 2 * j + (w >> 1);
    return bt[pi < a.max_pages ? pi : a.max_pages - 1];
  };
  auto dma_tiles = [&](int pg, int sb) {
    const unsigned short* kreg = a.cache + (((long)pg * a.HKV + kvh) * 2) * PAGE_ELEMS + 8 * lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 4 * w + i, sub = 4 * (w & 1) + i;  // 1 KB chunk of the tile / of the page region
      glds16(kreg + 512 * sub, smem[sb][0] + 1024 * ch);
      glds16(kreg + PAGE_ELEMS + 512 * sub, smem[sb][1] + 1024 * ch);
    }
  };

  // causal bound, and no tile wholly past the last real key ctx0 + n - 1
  const int ncausal = (ctx0 + q0 + QB) / KB, nreal = (ctx0 + n + KB - 1) / KB;
  const int ntile = ncausal < nreal ? ncausal : nreal;
  dma_tiles(page_of(0), 0);
  int pg_next = page_of(1 < ntile ? 1 : 0);
  // Q fragments and tile 0 complete before the loop (a vmcnt the waitcnt pass
  // sees, so it does not carry the Q loads into the loop header)
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
  __syncthreads();

  const float sl2 = a.sl2;
  const int qpos = ctx0 + qrow;  // this lane's position among the keys
  const int tau = swap34(l32);
  // byte offsets inside a page region: K unit (tau, 2ks + hh) = k_off + 512 ks,
  // V unit (2d + (l32 >> 4), 2sp + hh, l32 & 15) = v_off + 2048 d + 512 sp
  const int k_off = 16 * ((tau >> 4) * 256 + hh * 16 + (tau & 15));
  const int v_off = 16 * ((l32 >> 4) * 64 + hh * 16 + (l32 & 15));
  const bool wave_real = qw < n;  // a wave of padding rows only computes nothing

  for (int j = 0; j < ntile; ++j) {
    const int buf = j & 1;
    // the other buffer was released by the previous tile's barrier
    if (j + 1 < ntile) {
      dma_tiles(pg_next, buf ^ 1);
      pg_next = page_of(j + 2 < ntile ? j + 2 : j + 1);
    }
    const int kv0 = j * KB;
    if (wave_real && kv0 <= ctx0 + qw + 31) {
      const char* Ks = smem[buf][0] + k_off;
      const char* Vs = smem[buf][1] + v_off;
      // all 16 K fragments of the tile are read up front, so the QK^T MFMAs
      // never wait on one LDS read
      bf16x8 kf[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[t][ks] = *(const bf16x8*)(Ks + 8192 * t + 512 * ks);
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead (the scheduler sinks them otherwise)
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[t][ks], qf[ks], s[t], 0, 0, 0);
      }
      // the first half of the tile's V fragments is read now, so its LDS
      // latency hides under the softmax below; the second half is read under
      // the first half's P.V MFMAs
      bf16x8 vfr[4][2][2];
      auto read_v = [&](int d) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int sp = 0; sp < 2; ++sp) vfr[d][t][sp] = *(const bf16x8*)(Vs + 8192 * t + 2048 * d + 512 * sp);
      };
      read_v(0);
      read_v(1);
      __builtin_amdgcn_sched_barrier(0);
      if (kv0 + KB - 1 > ctx0 + qw) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // S^T row i = (r&3) + 8(r>>2) + 4hh is the page's token swap34(i)
            const int kv = kv0 + 32 * t + (r & 3) + 4 * hh + 16 * ((r >> 2) & 1) + 8 * (r >> 3);
            if (kv > qpos) s[t][r] = NEG;
          }
      }
      float mx = m;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
      mx = xor32_max(mx);
      // deferred rescale, as attention.hip: m only moves when a row's new max
      // exceeds it by more than RESCALE; the decision is wave-uniform
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
        pf[t][0] = pack_bf16x8(s[t], 0);
        pf[t][1] = pack_bf16x8(s[t], 8);
      }
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
  store(1.0f / l);
}

}  // namespace attnp
}  // namespace kgs

// q points at head 0 of Q row 0 (heads of a row are contiguous 128-element
// blocks, row stride ldq), cache at one layer's pages, o at [rows, >= H*128]
// with row stride ldo. block_tables int32 [nchunks, max_pages], desc int32
// [nchunks, 4] and qmap int32 [nqb, 2] are device arrays (kgs.ops.transformer
// paged_prefill_plan builds and validates them); their contents are trusted.
KGS_EXPORT int kgs_attn_prefill_paged_bf16(const void* q, const void* cache, const void* block_tables,
                                          const void* desc, const void* qmap, void* o, int nchunks, int nqb, int H,
                                          int HKV, int hd, int max_pages, long ldq, long ldo, float scale,
                                          hipStream_t s) {
  using namespace kgs::attnp;
  if (nchunks <= 0 || nqb <= 0 || H <= 0 || HKV <= 0 || H % HKV || max_pages <= 0) return KGS_ERR_SHAPE;
  if (hd != HD || nqb < nchunks) return KGS_ERR_SHAPE;
  if (ldq < (long)H * HD || ldo < (long)H * HD) return KGS_ERR_SHAPE;
  if (!q || !cache || !block_tables || !desc || !qmap || !o) return KGS_ERR_ALIGN;
  const uintptr_t al = (uintptr_t)q | (uintptr_t)cache | (uintptr_t)o;
  if ((al & 15) || ((ldq | ldo) & 7)) return KGS_ERR_ALIGN;
  if (((uintptr_t)block_tables | (uintptr_t)desc | (uintptr_t)qmap) & 3) return KGS_ERR_ALIGN;
  const long nwg = (long)nqb * H;
  if (nwg > 0x7fffffff) return KGS_ERR_SHAPE;
  Args a{(const unsigned short*)q, (const unsigned short*)cache, (const int*)block_tables, (const int*)desc,
         (const int*)qmap, (unsigned short*)o, ldq, ldo, H, HKV, max_pages, scale * 1.4426950408889634f};
  hipLaunchKernelGGL(fwd_paged, dim3((unsigned)nwg), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
