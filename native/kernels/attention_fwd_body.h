// Statement body of the flash-attention forward, included INSIDE a __global__
// function that has `Args a`, `constexpr bool LSE` and `float* lse` in scope:
// the production kernel kgs::attn::fwd (attention.hip, LSE false) and the
// training forward kgs::attn_train::fwd_lse (attention_train.hip), which also
// stores each query row's log-sum-exp into lse (fp32 [B*H, S], natural log).
// A textual include, not an inlined function: the production kernel's
// instruction stream is then the one the body had in attention.hip itself
// (an inlined function's by-value / by-reference Args changed its register
// allocation).
  __shared__ __attribute__((aligned(16))) char smem[2][2][TILE_BYTES];  // [buf][K, V]

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int nqb = a.S / QB;
  const int nwg = gridDim.x;
  // XCD-aware order: 8 consecutive dispatch slots of one XCD take 4 heads of
  // one KV group; work ids stay heaviest-first in dispatch time.
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
  const int qw = q0 + 32 * w;       // this wave's first query row
  const int qrow = qw + l32;        // this lane's query row
  const long tok0 = (long)b * a.S;     // first query token of the sequence
  const long ktok0 = (long)b * a.Sk;   // its first key token
  const int qoff = a.qoff;

  // Q fragments (B operand of S^T = K.Q^T): lane holds Q[qrow][16ks + 8hh .. +7]
  bf16x8 qf[8];
  {
    const bf16x8* qp = (const bf16x8*)(a.q + (tok0 + qrow) * a.ldq + (long)h * HD + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = qp[2 * ks];
  }

  const unsigned short* kbase = a.k + ktok0 * a.ldk + (long)kvh * HD;
  const unsigned short* vbase = a.v + ktok0 * a.ldv + (long)kvh * HD;
  // K/V tile jn -> LDS buffer sb by LDS-DMA (global_load_lds, no staging
  // registers): a 16 KB tile is 16 chunks of 1 KB = 4 rows of 256 B; wave w
  // issues chunks 4w .. 4w+3 of K and of V. Lane l lands at chunk + 16 l, i.e.
  // at slot (r, c') of the XOR image, so it fetches column c = c' ^ swz(r).
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

  const int ntile = a.causal ? (qoff + q0 + QB) / KB : a.Sk / KB;
  dma_tiles(0, 0);
  // Q fragments and tile 0 complete before the loop (a vmcnt the waitcnt pass
  // sees, so it does not carry the Q loads into the loop header)
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
  __syncthreads();

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = f32x16{};
  float m = NEG, l = 0.f;
  const float sl2 = a.sl2;

  // tr-read lane address pieces: group g = lane >> 4, lane 4q + p in it
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;

  for (int j = 0; j < ntile; ++j) {
    const int buf = j & 1;
    // the other buffer was released by the previous tile's barrier
    if (j + 1 < ntile) dma_tiles(j + 1, buf ^ 1);
    const int kv0 = j * KB;
    if (!a.causal || kv0 <= qoff + qw + 31) {
      const char* Ks = smem[buf][0];
      const char* Vs = smem[buf][1];
      // all 16 K fragments of the tile are read up front (the registers the
      // LDS-DMA staging freed), so the QK^T MFMAs never wait on one LDS read
      bf16x8 kf[2][8];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[t][ks] = *(const bf16x8*)(Ks + off(32 * t + l32, 2 * ks + hh));
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead (the scheduler sinks them otherwise)
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[t][ks], qf[ks], s[t], 0, 0, 0);
      }
      // the first half of the tile's V fragments is read now, so its LDS
      // latency hides under the softmax below (all 16 would spill at 2 waves
      // per SIMD); the second half is read under the first half's P.V MFMAs
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
      read_v(1);
      __builtin_amdgcn_sched_barrier(0);
      if (a.causal && kv0 + KB - 1 > qoff + qw) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (kv > qoff + qrow) s[t][r] = NEG;
          }
      }
      float mx = m;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
      mx = xor32_max(mx);  // v_permlane32_swap (kgs_common.h), not an LDS round trip
      // deferred rescale (guide T13): the running max m only moves when a row's
      // new max exceeds it by more than RESCALE (log2 units after sl2), so most
      // tiles skip the 64-multiply O rescale; p = exp2(s sl2 - m sl2) then stays
      // <= 2^RESCALE (fp32 sums and bf16 P are scale-free). Both l and O see the
      // same alpha, and the decision is wave-uniform, so no pending P.V is split.
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
    // ln sum exp(scale s) = (m sl2 + log2 l) ln 2; the 32 lanes of a half-wave
    // write 32 consecutive floats
    if (hh == 0)
      lse[((long)b * a.H + h) * a.S + qrow] = (m * sl2 + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
  }
  const float inv = 1.0f / l;
  unsigned short* op = a.o + (tok0 + qrow) * a.ldo + (long)h * HD;
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int dcol = 32 * d + 8 * r4 + 4 * hh;
      uint2 pk;
      pk.x = pack_bf16x2(o[d][4 * r4 + 0] * inv, o[d][4 * r4 + 1] * inv);
      pk.y = pack_bf16x2(o[d][4 * r4 + 2] * inv, o[d][4 * r4 + 3] * inv);
      *(uint2*)(op + dcol) = pk;
    }
