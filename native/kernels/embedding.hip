// Token embedding for gfx950: the row gather of the forward pass and a
// deterministic scatter-sum for its backward.
//
//   * embed_fwd : out[t, :] = bf16(scale * w[tok[t], :]); a token outside
//                 [0, vocab) gives a row of zeros (xent_fwd's convention for an
//                 ignored target); with scale == 1 the row is a bit copy
//   * embed_bwd : dw[v, :] = bf16(scale * sum_{t: tok[t] == v} dy[t, :]), dense:
//                 every element of [vocab, cols] is written exactly once, rows
//                 without a token as zeros, so the result does not depend on
//                 what dw held and needs no memset
//
// House rules (attention_train.hip): fp32 math, one bf16 rounding per output
// element, 16-B accesses, no float atomics, no workgroup waits on another.
//
// The backward's design. The caller passes the tokens' stable order: order[i] is
// the position of the i-th smallest token (equal tokens in ascending position)
// and sorted[i] = tok[order[i]]. The occurrences of a vocabulary row v are then
// the run sorted[lo .. hi) = v, and dw[v] is the sum of dy[order[lo .. hi)] taken
// in that order: ascending position, whatever the grid does.
//
// One wave owns RPW = 32 vocabulary rows and one 512-column slice of them (a
// lane owns one 16-B chunk of the slice). The issue's sketch has one wave per
// row find its run with two scalar binary searches; here the 64 lanes of a wave
// run the 64 searches of its 32 rows at once (lane k: the lower bound of row k,
// lane 32 + k: the lower bound of row k + 1's value, which is row k's upper
// bound), so a dense dw of 128256 rows costs 4008 searches per column slice
// instead of 128256, and the kernel's time is the time to write dw. The bounds
// then reach the row loop through v_readlane, which makes them wave-uniform:
// the walk over order[] is scalar loads, and UNR 16-B loads of dy are in flight
// before the first is added.
//
// The 32 rows of a wave are NOT consecutive: wave g owns g, g + G, g + 2 G, ...
// (G = ceil(vocab / 32) waves per slice). Frequent tokens tend to have
// neighbouring small ids (a Zipf-like vocabulary), and consecutive ownership
// would hand all the long runs to the first wave. A long run of ONE token is
// still summed by one wave per column slice, cols / 512 waves in all: the sum
// of a run is sequential by design (one order of additions), so its time grows
// with the run (profiles/r15/embedding/README.md has the all-same-token time).
//
// Grid, walk and summation order depend on (rows, vocab, cols) and on tok only:
// bitwise repeatable, capturable in a hipGraph, one launch, no workspace.
#include "kgs_common.h"

namespace kgs {
namespace emb {

// thread = one 16-B chunk of one output row (silu_mul_bwd's mapping)
__global__ __launch_bounds__(256) void embed_fwd(const unsigned short* __restrict__ w,
                                                 const long long* __restrict__ tok, unsigned short* __restrict__ out,
                                                 long rows, int cpr, long long vocab, long ldw, long ldo,
                                                 float scale) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * cpr) return;
  const long t = idx / cpr;
  const int c = (int)(idx - t * cpr);
  const long long v = tok[t];  // all 64 bits: 2^32 + 3 is out of range, not row 3
  bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (v >= 0 && v < vocab) {
    const bf16x8 x = ((const bf16x8*)(w + v * ldw))[c];
    if (scale == 1.0f) {
      o = x;
    } else {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = scale * bf2f((unsigned short)x[e]);
      o = pack_bf16x8(f, 0);
    }
  }
  ((bf16x8*)(out + t * ldo))[c] = o;
}

constexpr int RPW = 32;  // vocabulary rows per wave: lanes 0..31 hold their lower bounds, 32..63 their upper bounds
constexpr int UNR = 8;   // 16-B loads of dy in flight per lane

__device__ __forceinline__ void add_row(float (&acc)[8], const bf16x8 x) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] += bf2f((unsigned short)x[e]);
}

__global__ __launch_bounds__(256) void embed_bwd(const unsigned short* __restrict__ dy,
                                                 const long long* __restrict__ sorted,
                                                 const long long* __restrict__ order, unsigned short* __restrict__ dw,
                                                 int rows, long long vocab, int cpr, long lddy, long lddw, float scale,
                                                 long long pad, long long groups) {
  const int lane = threadIdx.x & 63;
  const long long g = 4LL * blockIdx.x + (threadIdx.x >> 6);  // wave-uniform
  if (g >= groups) return;
  const int c = (int)blockIdx.y * 64 + lane;
  const bool live = c < cpr;

  // lower_bound(sorted, key): the first i with sorted[i] >= key. Every probe is
  // at mid < rows; a key at or past vocab (the last wave's missing rows) is
  // searched like any other and never used.
  const long long key = g + (long long)(lane & 31) * groups + (lane >> 5);
  unsigned lo = 0, hi = (unsigned)rows;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (sorted[mid] < key) lo = mid + 1; else hi = mid;
  }
  const int bound = (int)lo;
  const long ldc = lddy / 8;  // dy's row stride in 16-B chunks (lddy % 8 == 0)

  for (int k = 0; k < RPW; ++k) {
    const long long v = g + (long long)k * groups;
    if (v >= vocab) break;
    const int b = __builtin_amdgcn_readlane(bound, k);
    const int e = v == pad ? b : __builtin_amdgcn_readlane(bound, RPW + k);
    if (live) {  // the readlanes above run with every lane active: k and v are wave-uniform
      bf16x8* dst = (bf16x8*)(dw + v * lddw) + c;
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const bf16x8* src = (const bf16x8*)dy + c;
      int i = b;
      for (; i + UNR <= e; i += UNR) {
        bf16x8 x[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) x[u] = __builtin_nontemporal_load(src + order[i + u] * ldc);
#pragma unroll
        for (int u = 0; u < UNR; ++u) add_row(acc, x[u]);
      }
      for (; i < e; ++i) add_row(acc, __builtin_nontemporal_load(src + order[i] * ldc));
      float o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = scale * acc[q];
      // no token, or the padding row: zero bits, whatever the sign of scale
      __builtin_nontemporal_store(b < e ? pack_bf16x8(o, 0) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0}, dst);
    }
  }
}

}  // namespace emb
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// w: bf16 [vocab, ldw]; tok: int64 [rows]; out: bf16 [rows, ldo] = bf16(scale *
// w[tok]), zeros for a token outside [0, vocab). Only columns < cols are written.
// rows == 0 is valid and launches nothing.
KGS_EXPORT int kgs_embed_fwd_bf16(const void* w, const void* tok, void* out, int rows, int vocab, int cols, long ldw,
                                 long ldo, float scale, hipStream_t s) {
  if (rows < 0 || vocab <= 0 || cols <= 0 || cols % 8 || ldw < cols || ldo < cols || ldw % 8 || ldo % 8)
    return KGS_ERR_ARG;
  if (!w || !al16(w) || !al16(out) || ((uintptr_t)tok & 7)) return KGS_ERR_ARG;
  if (rows == 0) return 0;
  if (!tok || !out) return KGS_ERR_ARG;
  const long n = (long)rows * (cols / 8);
  if ((n + 255) / 256 > 0x7fffffff) return KGS_ERR_SHAPE;
  hipLaunchKernelGGL(kgs::emb::embed_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     (const unsigned short*)w, (const long long*)tok, (unsigned short*)out, (long)rows, cols / 8,
                     (long long)vocab, ldw, ldo, scale);
  return (int)hipGetLastError();
}

// dy: bf16 [rows, lddy]; sorted, order: int64 [rows], the tokens in ascending
// order (equal tokens in ascending position) and the position each came from;
// dw: bf16 [vocab, lddw], every element of its [vocab, cols] written once
// whatever it held: bf16(scale * sum of the row's dy rows in order[]'s order),
// zeros for a row with no token and for row padding_idx (-1: none). One launch,
// nothing allocated, nothing zeroed beforehand. rows == 0 writes all zeros.
KGS_EXPORT int kgs_embed_bwd_bf16(const void* dy, const void* sorted, const void* order, void* dw, int rows, int vocab,
                                 int cols, long lddy, long lddw, float scale, long padding_idx, hipStream_t s) {
  if (rows < 0 || vocab <= 0 || cols <= 0 || cols % 8 || lddw < cols || lddw % 8) return KGS_ERR_ARG;
  if (!dw || !al16(dw)) return KGS_ERR_ARG;
  if (rows > 0 && (!dy || !sorted || !order || !al16(dy) || lddy < cols || lddy % 8)) return KGS_ERR_ARG;
  if (((uintptr_t)sorted & 7) || ((uintptr_t)order & 7)) return KGS_ERR_ARG;
  using namespace kgs::emb;
  const long long groups = ((long long)vocab + RPW - 1) / RPW;
  const long slices = ((long)(cols / 8) + 63) / 64;
  if (slices > 65535) return KGS_ERR_SHAPE;
  hipLaunchKernelGGL(embed_bwd, dim3((unsigned)((groups + 3) / 4), (unsigned)slices), dim3(256), 0, s,
                     (const unsigned short*)dy, (const long long*)sorted, (const long long*)order,
                     (unsigned short*)dw, rows, (long long)vocab, cols / 8, lddy, lddw, scale,
                     (long long)padding_idx, groups);
  return (int)hipGetLastError();
}
