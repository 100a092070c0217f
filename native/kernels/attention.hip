// Flash-attention forward for gfx950 (bf16 in/out, fp32 softmax/accumulate),
// head_dim 128, causal or full, GQA -- the prefill attention of the Llama
// stand-in (kgs/models/llama.py). Q, K and V are read in place from the fused
// QKV projection output ([tokens, (H + 2 HKV) * 128], any row stride) and O is
// written as [tokens, H * 128], the layout the O projection consumes: no
// transposes around the kernel.
//
// Structure (one workgroup = 4 waves = 128 query rows of one (batch, head);
// 2 workgroups per CU; K/V tiles of 64 keys):
//   * swapped QK^T on v_mfma_f32_32x32x16_bf16: S^T = K . Q^T, so a lane owns
//     ONE query row (lane & 31) and 32 of the tile's 64 scores -- the row max /
//     row sum are in-lane plus one xor-32 exchange, and the per-row rescale of
//     O is a lane scalar;
//   * the S^T accumulator is the B operand of P.V with no data movement
//     (O^T = V^T . P^T): registers 8s..8s+7 of each 32x32 tile are k-step s,
//     in the permuted key order kv = 16s + 8(j>>2) + 4(lane>>5) + (j&3) that
//     the V fragments are read in;
//   * V fragments via ds_read_b64_tr_b16 (a free transpose out of the
//     row-major tile), K fragments via ds_read_b128; both tiles use the
//     256-B-row XOR image off(r, c) = 256 r + 16 (c ^ ((r&3)<<2 | (r>>2)&3)),
//     conflict-free for the 16-lane groups of ds_read_b128 and the 32-lane
//     halves of the transposed read;
//   * double buffer filled by LDS-DMA: the next K/V tile's global_load_lds
//     are issued before the current tile's MFMAs (no staging registers),
//     vmcnt(0) + one barrier per tile;
//   * causal: fully-masked tiles are skipped per wave, the diagonal tiles are
//     masked in registers; q-blocks are dispatched heaviest first, and the four
//     query heads sharing a KV head are dealt to the same XCD back to back so
//     the K/V tiles they share are L2 hits.
#include "attention_fwd.h"

namespace kgs {
namespace attn {

__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void fwd(Args a) {
  constexpr bool LSE = false;
  float* const lse = nullptr;
#include "attention_fwd_body.h"
}

}  // namespace attn
}  // namespace kgs

// q/k/v/o point at head 0 of token 0 ([B*S, ld] token-major); heads of one
// token are contiguous 128-element blocks. Requires head_dim 128, S % 128 == 0,
// H % HKV == 0, 16-B aligned pointers and ld % 8 == 0.
//
// _ex: Sk keys per sequence ([B*Sk, ld] k/v), Sk >= S, Sk - S a multiple of 64:
// the S query rows are the LAST S positions of the sequence (a prefill chunk
// over Sk - S cached tokens), so causal row i sees keys 0 .. Sk - S + i.
KGS_EXPORT int kgs_attn_fwd_bf16_ex(const void* q, const void* k, const void* v, void* o, int B, int S, int Sk, int H,
                                   int HKV, int hd, long ldq, long ldk, long ldv, long ldo, float scale, int causal,
                                   hipStream_t s) {
  using namespace kgs::attn;
  if (B <= 0 || S <= 0 || H <= 0 || HKV <= 0 || H % HKV) return KGS_ERR_SHAPE;
  if (hd != HD || S % QB || Sk < S || (Sk - S) % KB) return KGS_ERR_SHAPE;
  if (ldq < (long)H * HD || ldk < (long)HKV * HD || ldv < (long)HKV * HD || ldo < (long)H * HD) return KGS_ERR_SHAPE;
  const uintptr_t al = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o;
  if ((al & 15) || (ldq | ldk | ldv | ldo) & 7) return KGS_ERR_ALIGN;
  const long nwg = (long)B * H * (S / QB);
  if (nwg > 0x7fffffff) return KGS_ERR_SHAPE;
  Args a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)o,
         ldq, ldk, ldv, ldo, B, S, H, HKV, scale * 1.4426950408889634f, causal ? 1 : 0, Sk, Sk - S};
  hipLaunchKernelGGL(fwd, dim3((unsigned)nwg), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

KGS_EXPORT int kgs_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, int B, int S, int H, int HKV,
                                int hd, long ldq, long ldk, long ldv, long ldo, float scale, int causal,
                                hipStream_t s) {
  return kgs_attn_fwd_bf16_ex(q, k, v, o, B, S, S, H, HKV, hd, ldq, ldk, ldv, ldo, scale, causal, s);
}
