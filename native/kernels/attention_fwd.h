// Types and helpers of the flash-attention forward (attention.hip describes the
// structure), shared with the training kernels (attention_train.hip). The
// kernel body itself is attention_fwd_body.h.
#pragma once
#include "kgs_common.h"

namespace kgs {
namespace attn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x4s __attribute__((ext_vector_type(4)));

constexpr int HD = 128;
constexpr int QB = 128;  // query rows per workgroup (4 waves x 32)
constexpr int KB = 64;   // keys per tile
constexpr int TILE_BYTES = KB * HD * 2;  // 16 KB
constexpr float NEG = -1.0e30f;
constexpr float RESCALE = 8.0f;  // deferred-max threshold, log2 units: P <= 256

struct Args {
  const unsigned short* q;
  const unsigned short* k;
  const unsigned short* v;
  unsigned short* o;
  long ldq, ldk, ldv, ldo;  // row strides (elements)
  int B, S, H, HKV;
  float sl2;  // softmax scale * log2(e)
  int causal;
  int Sk;    // keys per sequence (= S, or S + qoff for a chunk over a cached context)
  int qoff;  // position of query row 0 among the keys: causal row i sees keys <= qoff + i
};

__device__ __forceinline__ int swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int off(int r, int c) { return 256 * r + 16 * (c ^ swz(r)); }

__device__ __forceinline__ bf16x8 tr_frag(const char* lo, const char* hi) {
  const bf16x4s a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((KGS_LDS bf16x4s*)lo);
  const bf16x4s b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((KGS_LDS bf16x4s*)hi);
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& s, int base) { return pack_bf16x8(s, base); }

}  // namespace attn
}  // namespace kgs
