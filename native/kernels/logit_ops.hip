// Per-request logit operations of a serving step, on the device (gfx950):
// penalties from a token-count table that the sampling step itself keeps up to
// date, and the logprobs of the sampled token and the k most likely ones. With
// them a penalised or logprobs request needs nothing from the host that is not
// known before the previous token is read back. All three are memory-bound row
// passes (kgs.ops.transformer states the semantics in numpy:
// penalize_rows_reference, logprob_rows_reference).
//
//   kgs_penalize_rows_bf16   y = penalised copy of x, one 16-B chunk per thread
//   kgs_token_counts_add     counts[slot[j], tok[j]] += 1
//   kgs_logprob_rows_bf16    one 1024-thread workgroup per row, three passes over
//                            a row that stays in L2 after the first:
//     pass 1  row maximum (NaN detected) + count histogram of the keys' high bytes
//     pass 2  sum of exp(x - m) + count histogram of the low bytes inside the bin
//             of the k-th largest key -> the exact k-th largest logit
//     pass 3  the (at most 32) entries above the k-th key and its ties are
//             gathered into LDS and ranked there
//
// The count word w of counts[slot, token]: w & (2^30 - 1) is the token's count in
// the request's output, w & 2^30 marks a prompt token.
#include "row_select.h"

// penalize_rows is compared bit for bit with a float32 numpy statement: every
// operation below is rounded once (no fused multiply-add; `/` is hipcc's
// correctly rounded IEEE division, the HIP default)
#pragma clang fp contract(off)

namespace kgs {
namespace lop {

using namespace kgs::smp;

constexpr int KMAX = 32;
constexpr unsigned COUNT_MASK = (1u << 30) - 1;

__device__ __forceinline__ unsigned short penalize(unsigned short h, unsigned w, float freq, float pres, float rep) {
  if (w == 0) return h;
  float v = bf2f(h);
  const unsigned n = w & COUNT_MASK;
  if (n > 0) {
    const float a = freq * (float)n;
    const float t = a + pres;
    v = v - t;
  }
  if (rep != 1.f) v = (v > 0.f) ? v / rep : v * rep;
  return v != v ? (unsigned short)0x7fc0 : f2bf(v);  // a NaN result: the canonical quiet NaN
}

// grid (ceil(cols / 8 / 256), rows), 256 threads: thread = one 16-B chunk of x, two 16-B loads of count words
__global__ __launch_bounds__(256) void penalize_rows(const unsigned short* __restrict__ x,
                                                     unsigned short* __restrict__ y, const float* __restrict__ freq,
                                                     const float* __restrict__ pres, const float* __restrict__ rep,
                                                     const int* __restrict__ slot, const unsigned* __restrict__ counts,
                                                     int nslots, int cols, long ld) {
  const int row = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols / 8) return;
  const bf16x8 v = *((const bf16x8*)(x + row * ld) + c);
  bf16x8 o = v;
  const int s = slot[row];
  if (s >= 0 && s < nslots) {
    const uint4* wp = (const uint4*)(counts + (long)s * cols) + 2 * c;
    const uint4 w0 = wp[0], w1 = wp[1];
    const unsigned w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    if (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) {
      const float f = freq[row], p = pres[row], r = rep[row];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (short)penalize((unsigned short)v[e], w[e], f, p, r);
    }
  }
  *((bf16x8*)(y + (long)row * cols) + c) = o;
}

// one thread per row. Slots are unique within a launch, so the plain
// read-modify-write below has no other writer.
__global__ void token_counts_add(unsigned* __restrict__ counts, const long long* __restrict__ tok,
                                 const int* __restrict__ slot, int rows, int nslots, int cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  const int s = slot[j];
  const long long tk = tok[j];
  if (s < 0 || s >= nslots || tk < 0 || tk >= cols) return;
  counts[(long)s * cols + tk] += 1;
}

struct Shared {
  unsigned cnt[256 * NCOPY];
  unsigned bc[256];
  float sv[16];
  int si[16];
  int sel[4];
  float part[16];
  int wsum[16];
  unsigned ckey[KMAX];
  int cidx[KMAX];
  int npos;
};

__global__ __launch_bounds__(1024) void logprob_rows(const unsigned short* __restrict__ x,
                                                     const long long* __restrict__ tok, const int* __restrict__ want,
                                                     float* __restrict__ lp, float* __restrict__ top_val,
                                                     int* __restrict__ top_idx, int cols, long ld) {
  __shared__ Shared sh;
  const int row = blockIdx.x, t = threadIdx.x, cp = t & (NCOPY - 1);
  const int wk = want[row];
  if (wk < 0) return;
  const int k = min(min(wk, cols), KMAX);
  const unsigned short* xe = x + row * ld;
  const bf16x8* xr = (const bf16x8*)xe;
  const int nch = cols / 8;
  const long long tk = tok[row];
  float* tv = top_val + (long)row * KMAX;
  int* ti = top_idx + (long)row * KMAX;

  // pass 1: the maximum (NaN counts as the maximum) + the level-1 histogram
  if (k > 0) zero_counts(sh, t);
  if (t == 0) sh.npos = 0;
  __syncthreads();
  float bv = -INFINITY;
  int bi = NONE;
  for_chunks<false>(xr, nch, t, [&](int c, bf16x8 v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned short h = (unsigned short)v[e];
      const float f = bf2f(h);
      if (better(f, 8 * c + e, bv, bi)) bv = f, bi = 8 * c + e;
      if (k > 0) atomicAdd(&sh.cnt[(key16(h) >> 8) * NCOPY + cp], 1u);
    }
  });
  block_best(bv, bi, sh, t);
  const float m = bv;
  if (m != m || fabsf(m) == INFINITY) {  // a NaN in the row, or no finite maximum
    if (t == 0) lp[row] = __builtin_nanf("");
    if (t < k) tv[t] = __builtin_nanf(""), ti[t] = t;
    return;
  }

  unsigned hb = 0, inside = 0;
  if (k > 0) {
    hb = (unsigned)select_count(sh, (unsigned)k, inside, t);
    zero_counts(sh, t);
    __syncthreads();
  }

  // pass 2: sum of exp(x - m), this thread's elements in index order, + the level-2 histogram
  float acc = 0.f;
  for_chunks<false>(xr, nch, t, [&](int, bf16x8 v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned short h = (unsigned short)v[e];
      acc += expf(bf2f(h) - m);
      if (k > 0) {
        const unsigned key = key16(h);
        if ((key >> 8) == hb) atomicAdd(&sh.cnt[(key & 255) * NCOPY + cp], 1u);
      }
    }
  });
  // a fixed tree: lanes, then the 16 waves in order; every thread ends with the same sum
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((t & 63) == 0) sh.part[t >> 6] = acc;
  __syncthreads();
  float z = sh.part[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) z += sh.part[w];
  const float logz = logf(z);
  if (t == 0) lp[row] = (tk >= 0 && tk < cols) ? (bf2f(xe[tk]) - m) - logz : __builtin_nanf("");
  if (k == 0) return;

  // the k-th largest key, how many entries equal it (ties), and how many of them the k include (take)
  unsigned take;
  const unsigned lb = (unsigned)select_count(sh, inside, take, t);
  const unsigned kk = (hb << 8) | lb;
  const unsigned ties = sh.bc[lb];
  const bool ordered_ties = ties > take;  // more ties than places: the lowest indices win

  // pass 3: everything above the k-th key (fewer than k entries), and its ties when all of them fit
  for_chunks<false>(xr, nch, t, [&](int c, bf16x8 v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned key = key16((unsigned short)v[e]);
      if (ordered_ties ? key > kk : key >= kk) {
        const int pos = atomicAdd(&sh.npos, 1);
        if (pos < KMAX) sh.ckey[pos] = key, sh.cidx[pos] = 8 * c + e;
      }
    }
  });
  if (ordered_ties) {
    // Thread t takes the contiguous chunks [t * cpt, (t + 1) * cpt): the ties
    // before a thread's range are then the ties of the threads before it.
    const int cpt = (nch + NT - 1) / NT;
    const int c0 = min(t * cpt, nch), c1 = min(c0 + cpt, nch);
    int mine = 0;
    for (int c = c0; c < c1; ++c) {
      const bf16x8 v = xr[c];
#pragma unroll
      for (int e = 0; e < 8; ++e) mine += key16((unsigned short)v[e]) == kk;
    }
    int incl = mine;  // inclusive scan: the wave, then the waves before it
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if ((t & 63) >= o) incl += up;
    }
    if ((t & 63) == 63) sh.wsum[t >> 6] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int w = 0; w < (t >> 6); ++w) before += sh.wsum[w];
    if (mine > 0 && before < (int)take) {
      const int base = k - (int)take;  // the entries above the k-th key come first
      for (int c = c0; c < c1; ++c) {
        const bf16x8 v = xr[c];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (key16((unsigned short)v[e]) == kk) {
            if (before < (int)take) sh.ckey[base + before] = kk, sh.cidx[base + before] = 8 * c + e;
            ++before;
          }
      }
    }
  }
  __syncthreads();
  // rank the k entries: key descending, then index ascending
  if (t < k) {
    const unsigned key = sh.ckey[t];
    const int idx = sh.cidx[t];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += sh.ckey[j] > key || (sh.ckey[j] == key && sh.cidx[j] < idx);
    tv[rank] = (bf2f(xe[idx]) - m) - logz;
    ti[rank] = idx;
  }
}

}  // namespace lop
}  // namespace kgs

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// x: [rows, ld] bf16 (cols % 8 == 0, ld % 8 == 0, 16-B aligned); y: [rows, cols] bf16, contiguous, 16-B aligned;
// freq / pres / rep: fp32 [rows]; slot: int32 [rows] (< 0 or >= nslots: the row is copied);
// counts: int32 [nslots, cols], 16-B aligned
KGS_EXPORT int kgs_penalize_rows_bf16(const void* x, void* y, const float* freq, const float* pres, const float* rep,
                                      const int* slot, const void* counts, int rows, int cols, long ld, int nslots,
                                      hipStream_t s) {
  if (rows < 0 || cols <= 0 || ld < cols || nslots < 0) return KGS_ERR_SHAPE;
  if (cols % 8 || ld % 8 || !al16(x) || !al16(y) || !al16(counts)) return KGS_ERR_ALIGN;
  if (rows == 0) return 0;
  if (rows > 65535) return KGS_ERR_SHAPE;
  if (!x || !y || !freq || !pres || !rep || !slot || (nslots > 0 && !counts)) return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::lop::penalize_rows, dim3((cols / 8 + 255) / 256, rows), dim3(256), 0, s,
                     (const unsigned short*)x, (unsigned short*)y, freq, pres, rep, slot, (const unsigned*)counts,
                     nslots, cols, ld);
  return (int)hipGetLastError();
}

// counts: int32 [nslots, cols]; tok: int64 [rows]; slot: int32 [rows]. counts[slot[j], tok[j]] += 1 where
// 0 <= slot[j] < nslots and 0 <= tok[j] < cols; nothing is written otherwise. The slots >= 0 of one launch
// must be distinct (the engine gives each request its own): the update is not atomic.
KGS_EXPORT int kgs_token_counts_add(void* counts, const long long* tok, const int* slot, int rows, int nslots,
                                    int cols, hipStream_t s) {
  if (rows < 0 || cols <= 0 || nslots < 0) return KGS_ERR_SHAPE;
  if (rows == 0 || nslots == 0) return 0;
  if (!counts || !tok || !slot) return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::lop::token_counts_add, dim3((rows + 255) / 256), dim3(256), 0, s, (unsigned*)counts, tok,
                     slot, rows, nslots, cols);
  return (int)hipGetLastError();
}

// logits: [rows, ld] bf16 (cols % 8 == 0, ld % 8 == 0, 16-B aligned); tok: int64 [rows]; want: int32 [rows]
// (< 0: the row is skipped, else k = min(want, cols, 32)); lp: fp32 [rows]; top_val: fp32 [rows, 32];
// top_idx: int32 [rows, 32]. Entries past k and skipped rows are left untouched.
KGS_EXPORT int kgs_logprob_rows_bf16(const void* logits, const long long* tok, const int* want, float* lp,
                                     float* top_val, int* top_idx, int rows, int cols, long ld, hipStream_t s) {
  if (rows < 0 || cols <= 0 || ld < cols) return KGS_ERR_SHAPE;
  if (cols % 8 || ld % 8 || !al16(logits)) return KGS_ERR_ALIGN;
  if (rows == 0) return 0;
  if (!logits || !tok || !want || !lp || !top_val || !top_idx) return KGS_ERR_ARG;
  hipLaunchKernelGGL(kgs::lop::logprob_rows, dim3(rows), dim3(kgs::smp::NT), 0, s, (const unsigned short*)logits, tok,
                     want, lp, top_val, top_idx, cols, ld);
  return (int)hipGetLastError();
}
