// v224_fused.hip.inc -- register-resident radix-2^K ACS pass (included by v224_hip.hip).
//
// One launch runs K trellis steps (port.c:168-181, K times).  Let XB = 23 - K.  After t steps of
// a pass a 23-bit state number is  S = [ q_lo : x : q_hi ]  with q = [q_lo|q_hi] a K-bit "physical"
// index that never changes for a given storage slot, q_hi = the top t bits of q, q_lo the rest:
//      t = 0 :  S = q << XB | x          (how the pass reads  old[])
//      t = K :  S = x << K  | q          (how the pass writes new[])
// Step t+1 pairs the two slots whose q differ in bit (K-1-t) (that bit is S's MSB) and leaves the
// two survivors in the same two slots: an in-place butterfly network, bit K-1 first, bit 0 last.
// A thread owns ALL 2^K slots of two neighbouring x (packed lo/hi in one VGPR per slot), so every
// butterfly is register-to-register, with v_pk_* u16 arithmetic doing both x at once; no LDS, no
// cross-lane traffic.  Per launch the metrics move through HBM once (32 MiB) instead of K times.
//
// Arithmetic.  With c = 255 + e the port's four candidates (port.c:171-176) are
//      oi + 255 +/- e,  oj + 255 -/+ e,        e = (i odd ? s0 + s1 - 255 : s0 - s1),
// sign flipped when parity(2i & POLY1) = 1.  The common 255 is dropped (V224Dev::off accounts for
// it), so a butterfly is  n0 = min(oi + E, oj - E),  n1 = min(oi - E, oj + E)  with E = +/-e.  The
// parity splits into an x part (per lane and half, one popcount per stage) and a q part that is a
// compile-time constant of the unrolled code.  Metrics are unsigned and windowed (entry minimum
// = V224_BASE), so u16 min is exact and the decision is the sign bit of the u16 difference:
// bit15(A - B) = 1  <=>  A < B  <=>  the MSB-clear predecessor survives (port decision 0; ties go
// to the MSB-set predecessor as ">= 0" does in port.c:178).  Rows therefore store NOT(decision).
//
// Decision row layout for meta = (K << 8) | stage  (1 MiB per row for every K):
//      x = tid*2 + h ;  q_out = physical slot of the NEW state;  g = q_out >> 4, pos = q_out & 15
//      K >= 4 : dword[tid * 2^(K-4) + g], bit 16*h + pos
//      K == 3 : u16[tid], bit 8*h + q_out          K == 2 : u8[tid], bit 4*h + q_out
#pragma once
#include <utility>

#define FUSED_MAX_K      7
#define FUSED_DEFAULT_K  5

typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2u16 as_v2(unsigned x) { return __builtin_bit_cast(v2u16, x); }
__device__ __forceinline__ unsigned as_u32(v2u16 x) { return __builtin_bit_cast(unsigned, x); }

__host__ __device__ constexpr unsigned cpar(unsigned x) { return (unsigned)__builtin_parity(x); }

#define V224_P1H (V224_POLY1 >> 1)     // parity(2i & POLY1) == parity(i & P1H)

// static (q-dependent) part of the branch parity at stage t (0-based), slot q with pair bit clear
template <int K>
__host__ __device__ constexpr unsigned q_parity(int t, unsigned q) {
  const int XB = V224_SBITS - K;
  unsigned qlo = q & ((1u << (K - t)) - 1u), qhi = q >> (K - t);
  return cpar(((qlo << (t + XB)) & V224_P1H)) ^ cpar(qhi & V224_P1H);
}

template <int K> struct FusedCfg {
  static constexpr int XB = V224_SBITS - K;
  static constexpr int NQ = 1 << K;
  static constexpr int NW = (K >= 4) ? (1 << (K - 4)) : 1;
};

// one butterfly; every index is a compile-time constant so r[] and acc[] stay in VGPRs
template <int K, int T, int QQ>
__device__ __forceinline__ void fused_bfly(v2u16 (&r)[1 << K], unsigned (&acc)[FusedCfg<K>::NW],
                                           const v2u16 E0, const v2u16 E1) {
  constexpr int NW = FusedCfg<K>::NW;
  constexpr int pb = K - 1 - T;
  constexpr unsigned q = (((unsigned)QQ >> pb) << (pb + 1)) | ((unsigned)QQ & ((1u << pb) - 1u));
  constexpr unsigned qj = q | (1u << pb);
  constexpr unsigned sgn = q_parity<K>(T, q);
  constexpr unsigned i0 = (T == 0) ? 0u : ((q >> (K - T)) & 1u);
  const v2u16 E = i0 ? E1 : E0;
  const v2u16 oi = r[q], oj = r[qj];
  v2u16 A, B, C, D;
  if constexpr (sgn != 0) { A = oi - E; B = oj + E; C = oi + E; D = oj - E; }
  else                    { A = oi + E; B = oj - E; C = oi - E; D = oj + E; }
  const v2u16 dab = A - B, dcd = C - D;
  r[q]  = __builtin_elementwise_min(A, B);
  r[qj] = __builtin_elementwise_min(C, D);
  const unsigned nb0 = as_u32(dab >> (unsigned short)15);    // 1 per half where A < B
  const unsigned nb1 = as_u32(dcd >> (unsigned short)15);
  constexpr unsigned g0 = (q >> 4) % NW, g1 = (qj >> 4) % NW;
  acc[g0] |= nb0 << (q & 15u);
  acc[g1] |= nb1 << (qj & 15u);
}

template <int K, int T, int... QQ>
__device__ __forceinline__ void fused_bflies(v2u16 (&r)[1 << K], unsigned (&acc)[FusedCfg<K>::NW],
                                             const v2u16 E0, const v2u16 E1,
                                             std::integer_sequence<int, QQ...>) {
  (fused_bfly<K, T, QQ>(r, acc, E0, E1), ...);
}

typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));

// plain 16- / 8-byte stores at a 32-bit byte offset from base
__device__ __forceinline__ void store16(uint32_t *base, unsigned off_bytes, v4u32 v) {
  *reinterpret_cast<v4u32 *>(reinterpret_cast<char *>(base) + off_bytes) = v;
}
__device__ __forceinline__ void store8(uint32_t *base, unsigned off_bytes, v2u32 v) {
  *reinterpret_cast<v2u32 *>(reinterpret_cast<char *>(base) + off_bytes) = v;
}

template <int K, int T>
__device__ __forceinline__ void fused_stage(v2u16 (&r)[1 << K], const unsigned tid,
                                            const uint8_t *__restrict__ syms,
                                            uint32_t *__restrict__ row) {
  constexpr int XB = FusedCfg<K>::XB, NQ = FusedCfg<K>::NQ, NW = FusedCfg<K>::NW;
  const int s0 = syms[2 * T], s1 = syms[2 * T + 1];
  const int e0 = s0 - s1, e1 = s0 + s1 - 255;
  // x part of the parity: (x << T) against P1H
  constexpr unsigned mt = (V224_P1H >> T) & ((1u << XB) - 1u);
  const unsigned pxl = __popc((2u * tid) & mt) & 1u;
  const unsigned pxh = pxl ^ (mt & 1u);
  unsigned E0u, E1u;                 // lo half = x even, hi half = x odd
  if constexpr (T == 0) {            // i & 1 == x & 1 == half index: lo uses e0, hi uses e1
    E0u = ((unsigned)(pxl ? -e0 : e0) & 0xffffu) | ((unsigned)(pxh ? -e1 : e1) << 16);
    E1u = E0u;
  } else {
    E0u = ((unsigned)(pxl ? -e0 : e0) & 0xffffu) | ((unsigned)(pxh ? -e0 : e0) << 16);
    E1u = ((unsigned)(pxl ? -e1 : e1) & 0xffffu) | ((unsigned)(pxh ? -e1 : e1) << 16);
  }
  unsigned acc[NW];
#pragma unroll
  for (int g = 0; g < NW; g++) acc[g] = 0;
  fused_bflies<K, T>(r, acc, as_v2(E0u), as_v2(E1u), std::make_integer_sequence<int, NQ / 2>{});

  if constexpr (K >= 6) {
#pragma unroll
    for (int g = 0; g < NW; g += 4) {
      v4u32 v = { acc[g], acc[g + 1], acc[g + 2], acc[g + 3] };
      store16(row, (tid * NW + g) * 4, v);
    }
  } else if constexpr (K == 5) {
    v2u32 v = { acc[0], acc[1] };
    store8(row, tid * 8, v);
  } else if constexpr (K == 4) {
    row[tid] = acc[0];
  } else if constexpr (K == 3) {
    reinterpret_cast<uint16_t *>(row)[tid] = (uint16_t)((acc[0] & 0xffu) | ((acc[0] >> 8) & 0xff00u));
  } else {
    reinterpret_cast<uint8_t *>(row)[tid] = (uint8_t)((acc[0] & 0xfu) | ((acc[0] >> 12) & 0xf0u));
  }
}

template <int K, int... T>
__device__ __forceinline__ void fused_stages(v2u16 (&r)[1 << K], const unsigned tid,
                                             const uint8_t *__restrict__ syms,
                                             uint32_t *__restrict__ rows, int row0,
                                             std::integer_sequence<int, T...>) {
  (fused_stage<K, T>(r, tid, syms, rows + (size_t)(row0 + T) * V224_ROWWORDS), ...);
}

template <int K>
__global__ __launch_bounds__(256) void k_acs_fused(const uint32_t *__restrict__ oldm,
                                                   uint32_t *__restrict__ newm,
                                                   uint32_t *__restrict__ rows, int row0,
                                                   const uint8_t *__restrict__ syms, V224Dev *ds,
                                                   unsigned pass, uint32_t *rowmeta) {
  constexpr int XB = FusedCfg<K>::XB, NQ = FusedCfg<K>::NQ;
  const unsigned tid = blockIdx.x * 256 + threadIdx.x;          // owns x = 2*tid, 2*tid + 1

  v2u16 r[NQ];
  {
    const uint32_t *src = oldm + tid;                           // old[(q << XB) + 2*tid .. +1]
#pragma unroll
    for (int q = 0; q < NQ; q++) r[q] = as_v2(src[(size_t)q << (XB - 1)]);
  }
  // the metric loads above are in flight while the workgroup reduces last launch's minima
  const unsigned adj = input_min(ds, pass) - V224_BASE;
  const v2u16 adj2 = as_v2((adj & 0xffffu) * 0x10001u);   // adj may be negative: keep 16 bits per half
#pragma unroll
  for (int q = 0; q < NQ; q++) r[q] -= adj2;

  fused_stages<K>(r, tid, syms, rows, row0, std::make_integer_sequence<int, K>{});

  // write new[(x << K) + q]: lo halves of r[0..NQ) then hi halves, 4*NQ contiguous bytes per thread
  v2u16 mnv = r[0];
#pragma unroll
  for (int q = 1; q < NQ; q++) mnv = __builtin_elementwise_min(mnv, r[q]);
  uint32_t *dst = newm + (size_t)tid * NQ;
  if constexpr (NQ >= 8) {
#pragma unroll
    for (int q = 0; q < NQ; q += 8) {
      uint4 lo, hi;
      lo.x = __builtin_amdgcn_perm(as_u32(r[q + 1]), as_u32(r[q + 0]), 0x05040100u);
      lo.y = __builtin_amdgcn_perm(as_u32(r[q + 3]), as_u32(r[q + 2]), 0x05040100u);
      lo.z = __builtin_amdgcn_perm(as_u32(r[q + 5]), as_u32(r[q + 4]), 0x05040100u);
      lo.w = __builtin_amdgcn_perm(as_u32(r[q + 7]), as_u32(r[q + 6]), 0x05040100u);
      hi.x = __builtin_amdgcn_perm(as_u32(r[q + 1]), as_u32(r[q + 0]), 0x07060302u);
      hi.y = __builtin_amdgcn_perm(as_u32(r[q + 3]), as_u32(r[q + 2]), 0x07060302u);
      hi.z = __builtin_amdgcn_perm(as_u32(r[q + 5]), as_u32(r[q + 4]), 0x07060302u);
      hi.w = __builtin_amdgcn_perm(as_u32(r[q + 7]), as_u32(r[q + 6]), 0x07060302u);
      store16(newm, (tid * NQ + (q >> 1)) * 4, v4u32{ lo.x, lo.y, lo.z, lo.w });
      store16(newm, (tid * NQ + (NQ >> 1) + (q >> 1)) * 4, v4u32{ hi.x, hi.y, hi.z, hi.w });
    }
  } else {   // K == 2: 4 slots -> 2 dwords per half
    uint4 v;
    v.x = __builtin_amdgcn_perm(as_u32(r[1]), as_u32(r[0]), 0x05040100u);
    v.y = __builtin_amdgcn_perm(as_u32(r[3]), as_u32(r[2]), 0x05040100u);
    v.z = __builtin_amdgcn_perm(as_u32(r[1]), as_u32(r[0]), 0x07060302u);
    v.w = __builtin_amdgcn_perm(as_u32(r[3]), as_u32(r[2]), 0x07060302u);
    reinterpret_cast<uint4 *>(dst)[0] = v;
  }

  unsigned mn = (unsigned)mnv.x < (unsigned)mnv.y ? (unsigned)mnv.x : (unsigned)mnv.y;
  mn = wave_min_u32(mn);
  output_min(ds, pass, mn, (long long)(int)adj + 255ll * K);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int t = 0; t < K; t++) rowmeta[row0 + t] = ((unsigned)K << 8) | (unsigned)(t + 1);
}

// decision for NEW state `s` of a row written by stage `stage` of a K-step pass
__device__ __forceinline__ unsigned fused_get_decision(const uint32_t *__restrict__ r, unsigned meta,
                                                       unsigned s) {
  const unsigned K = meta >> 8, tau = meta & 0xffu, XB = V224_SBITS - K;
  const unsigned x = (s >> tau) & ((1u << XB) - 1u);
  const unsigned qout = ((s & ((1u << tau) - 1u)) << (K - tau)) | (s >> (XB + tau));
  const unsigned tid = x >> 1, h = x & 1u;
  unsigned nb;
  if (K >= 4) {
    const unsigned w = r[(tid << (K - 4)) + (qout >> 4)];
    nb = (w >> (16u * h + (qout & 15u))) & 1u;
  } else if (K == 3) {
    nb = ((unsigned)reinterpret_cast<const uint16_t *>(r)[tid] >> (8u * h + qout)) & 1u;
  } else {
    nb = ((unsigned)reinterpret_cast<const uint8_t *>(r)[tid] >> (4u * h + qout)) & 1u;
  }
  return nb ^ 1u;
}

static int fused_launch(int k, const uint16_t *oldm, uint16_t *newm, uint32_t *rows, int row0,
                        const uint8_t *syms, V224Dev *ds, unsigned pass, uint32_t *rowmeta,
                        hipStream_t st) {
  const uint32_t *o = reinterpret_cast<const uint32_t *>(oldm);
  uint32_t *n = reinterpret_cast<uint32_t *>(newm);
#define FUSED_CASE(KK)                                                                        \
  case KK:                                                                                    \
    k_acs_fused<KK><<<(1u << (V224_SBITS - KK - 1)) / 256, 256, 0, st>>>(o, n, rows, row0, syms, ds, pass, rowmeta); \
    break;
  switch (k) {
    case 1:
      k_acs_simple<<<V224_NSTATES / 32 / 256, 256, 0, st>>>(oldm, newm, rows + (size_t)row0 * V224_ROWWORDS,
                                                           syms, ds, pass, rowmeta, row0);
      break;
      FUSED_CASE(2) FUSED_CASE(3) FUSED_CASE(4) FUSED_CASE(5) FUSED_CASE(6) FUSED_CASE(7)
    default: return -1;
  }
#undef FUSED_CASE
  return 0;
}
