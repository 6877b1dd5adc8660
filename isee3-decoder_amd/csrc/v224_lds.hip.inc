// v224_lds.hip.inc -- LDS-staged two-level ACS pass: 8 trellis steps per launch (engine LDS).
//
// Same index algebra as v224_fused.hip.inc with K = 8 (XB = 15): a launch reads old[(q << 15) + x]
// and writes new[(x << 8) + q], q = 8-bit physical slot.  A 512-thread workgroup owns a TILE = all
// 256 slots x 64 consecutive x = 16 384 states = 32 KiB, staged in LDS as [q][x] (128-byte rows):
//
//   load     256 runs of 128 B from HBM (global_load_dwordx4, 8 lanes per run) -> LDS, linear
//   level 1  thread (q_low4, x pair) pulls its 16 slots {q_high4} into VGPRs (ds_read_b32, 256 B
//            contiguous per wave instruction), runs steps 1-4 (pair bits 7,6,5,4) register to
//            register with packed u16 math, and puts them back in place
//   level 2  thread (q_high4, x pair) pulls its 16 slots {q_low4}, runs steps 5-8 (pair bits 3..0)
//   store    (x, x+1) packing is re-paired to (q, q+1) with v_perm, written to a second LDS image
//            [x][q] (XOR-swizzled 16-byte chunks), and streamed out lane-contiguous: the tile's
//            output is one contiguous 32 KiB block of new[]
//
// Threads carry 16 metric VGPRs instead of 32-64, so the grid is 512 workgroups x 8 waves = 4 waves
// per SIMD (the register-only kernel has 1-2), metric traffic falls to 32 MiB per 8 steps, and every
// global access is a full 128-byte line.  Decisions: one dword per thread and stage
// (bit 16h + slot-in-thread), row word index tile*512 + thread.
#pragma once

#define LDS8_META(tau) ((1u << 16) | (8u << 8) | (unsigned)(tau))

// position of physical slot bit j inside the state number after t steps (K = 8, XB = 15)
__host__ __device__ constexpr int lds8_qpos(int j, int t) { return j >= 8 - t ? j - (8 - t) : j + t + 15; }
// mask over slot bits j: parity contribution of bit j at stage t (pair bit excluded: it is clear
// for the butterfly's MSB-clear predecessor)
__host__ __device__ constexpr unsigned lds8_qmask(int t) {
  unsigned m = 0;
  for (int j = 0; j < 8; j++)
    if (j != 7 - t && ((V224_P1H >> lds8_qpos(j, t)) & 1u)) m |= 1u << j;
  return m;
}

// One packed butterfly (two x at once), the port's own candidates  old + bm  /  old + 510 - bm
// (port.c:171-176) in packed u16.  Measured on gfx950 (scratch/valu_rate.hip): VOP3P packed ops and
// three-operand VOP3 ops (v_bfi, v_and_or, v_lshl_or, v_perm ...) issue at 4 cycles per wave64, plain VOP2
// (v_add_u32, v_and, v_lshrrev ...) at 2.  (A - B) has bit 15 / 31 = (A < B) = NOT(port decision): rows hold
// the complement (ties: A == B gives 0 = decision 1, as ">= 0" does in port.c:178).
// Decisions are gathered into one dword per stage, each stage into its own row: insert k of the stage
// (k = 2*butterfly + which output) sits at bit k (low half = even x) and 16 + k (odd x).
#define LDS8_STAGGER 2     // measured: 15.31 -> 14.83 us per launch (1: 15.29, 3: 15.04, 4: 14.95, 6: 16.24)
template <int T, int BF>
__device__ __forceinline__ void lds8_bfly(v2u16 (&r)[16], unsigned &acc, const unsigned C0, const unsigned N0,
                                          const unsigned C1, const unsigned N1) {
  constexpr int LEVEL = T / 4, lb = 3 - (T % 4);
  constexpr unsigned rq = (((unsigned)BF >> lb) << (lb + 1)) | ((unsigned)BF & ((1u << lb) - 1u));
  constexpr unsigned rj = rq | (1u << lb);
  constexpr unsigned qreg = LEVEL == 0 ? (rq << 4) : rq;        // the register index as slot bits
  constexpr unsigned sgn = cpar(qreg & lds8_qmask(T));
  // i & 1 of the MSB-clear predecessor = slot bit 8-T (T >= 1); static when that bit is a register bit
  constexpr bool i0_static = (T >= 1) && (LEVEL == 0 ? true : (T >= 5));
  constexpr unsigned i0 = i0_static ? ((qreg >> (8 - T)) & 1u) : 0u;
  const unsigned bc = i0 ? C1 : C0, bn = i0 ? N1 : N0;          // bm and 510 - bm, per half
  const unsigned cc = sgn ? bn : bc, cn = sgn ? bc : bn;        // register parity swaps the roles
  const unsigned oi = as_u32(r[rq]), oj = as_u32(r[rj]);
  const v2u16 Av = as_v2(oi) + as_v2(cc), Bv = as_v2(oj) + as_v2(cn), Cv = as_v2(oi) + as_v2(cn), Dv = as_v2(oj) + as_v2(cc);
  const unsigned A = as_u32(Av), B = as_u32(Bv), C = as_u32(Cv), D = as_u32(Dv);
  const unsigned d0 = as_u32(Av - Bv), d1 = as_u32(Cv - Dv);   // bit 15 / 31 = (A < B) = NOT decision
  r[rq] = __builtin_elementwise_min(as_v2(A), as_v2(B));
  r[rj] = __builtin_elementwise_min(as_v2(C), as_v2(D));
  // insert k of the stage lands at bit k / 16 + k: independent shifts, no serial chain
  acc |= (d0 & 0x80008000u) >> (15 - 2 * BF);
  acc |= (d1 & 0x80008000u) >> (14 - 2 * BF);
}

template <int T, int... BF>
__device__ __forceinline__ void lds8_bflies(v2u16 (&r)[16], unsigned &acc, const unsigned C0, const unsigned N0,
                                            const unsigned C1, const unsigned N1, std::integer_sequence<int, BF...>) {
  (lds8_bfly<T, BF>(r, acc, C0, N0, C1, N1), ...);
}

// one trellis step on the 16 slots a thread holds; qthr = the thread's own slot bits (in place),
// xe = the even x of its pair
template <int T>
__device__ __forceinline__ unsigned lds8_stage(v2u16 (&r)[16], const unsigned qthr, const unsigned xe,
                                               const uint8_t *__restrict__ syms) {
  const unsigned s0 = syms[2 * T], s1 = syms[2 * T + 1];
  const unsigned c0 = s0 + 255u - s1, c1 = s0 + s1;            // port.c:170 for i even / odd
  constexpr unsigned xmask = (V224_P1H >> T) & 0x7fffu;
  constexpr unsigned qmask = lds8_qmask(T);
  const unsigned pl = (__popc(qthr & qmask) + __popc(xe & xmask)) & 1u;
  const unsigned ph = pl ^ (xmask & 1u);
  unsigned C0, C1;                                               // bm per half: low = even x, high = odd x
  if constexpr (T == 0) {                 // i & 1 = x & 1 = half index
    C0 = (pl ? 510u - c0 : c0) | ((ph ? 510u - c1 : c1) << 16);
    C1 = C0;
  } else if constexpr (T == 4) {          // i & 1 = slot bit 4 = lowest bit of the thread's q_high
    const unsigned c = ((qthr >> 4) & 1u) ? c1 : c0;
    C0 = (pl ? 510u - c : c) | ((ph ? 510u - c : c) << 16);
    C1 = C0;
  } else {
    C0 = (pl ? 510u - c0 : c0) | ((ph ? 510u - c0 : c0) << 16);
    C1 = (pl ? 510u - c1 : c1) | ((ph ? 510u - c1 : c1) << 16);
  }
  const unsigned N0 = 0x01fe01feu - C0, N1 = 0x01fe01feu - C1;   // 510 - bm per half (no borrow: bm <= 510)
  unsigned acc = 0;
  lds8_bflies<T>(r, acc, C0, N0, C1, N1, std::make_integer_sequence<int, 8>{});
  return acc;
}

// minimum of the previous launch's per-workgroup minima, reduced cooperatively by the 8 waves
// (a variant where every wave reduces all entries on its own, saving this barrier, measured slower)
__device__ __forceinline__ unsigned block_min512_in(const V224Dev *ds, unsigned pass, unsigned *s8) {
  const unsigned *a = ds->blkmin[pass & 1];
  const unsigned n = ds->nmin[pass & 1];
  unsigned m = 0xffffffffu;
  for (unsigned i = threadIdx.x; i < n; i += 512) { unsigned v = a[i]; m = v < m ? v : m; }
  m = wave_min_u32(m);
  if ((threadIdx.x & 63) == 0) s8[threadIdx.x >> 6] = m;
  __syncthreads();
  unsigned r = s8[0];
#pragma unroll
  for (int w = 1; w < 8; w++) r = s8[w] < r ? s8[w] : r;
  return r;
}

// ---- one tile, from the LDS input image to the global stores ------------------------------------
// `in` holds the tile as [q][x]; on return the tile's new metrics and decisions have been issued to
// global memory (asynchronously) and `in` may be refilled.  Returns the packed minimum of the outputs.
__device__ __forceinline__ v2u16 lds8_tile(unsigned char *in, unsigned char *outb, const unsigned ti, const v2u16 adj2,
                                           uint16_t *__restrict__ newm, uint32_t *__restrict__ rows, int row0,
                                           const uint8_t *__restrict__ syms) {
  const unsigned th = threadIdx.x;
  const unsigned xp = th & 31, qt = th >> 5;            // x pair, and the thread's 4 slot bits
  const unsigned xe = ti * 64 + 2 * xp;
  uint32_t *rb = rows + (size_t)row0 * V224_ROWWORDS + ti * 512 + th;
  v2u16 r[16];

  // level 1: slots (qa << 4) | qt
#pragma unroll
  for (int a = 0; a < 16; a++) r[a] = as_v2(*reinterpret_cast<const unsigned *>(in + (((a << 4) | qt) * 128 + xp * 4))) - adj2;
  {
    uint4 dv;
    dv.x = lds8_stage<0>(r, qt, xe, syms);
    dv.y = lds8_stage<1>(r, qt, xe, syms);
    dv.z = lds8_stage<2>(r, qt, xe, syms);
    dv.w = lds8_stage<3>(r, qt, xe, syms);
    rb[0] = dv.x; rb[V224_ROWWORDS] = dv.y; rb[2 * V224_ROWWORDS] = dv.z; rb[3 * V224_ROWWORDS] = dv.w;
  }
#pragma unroll
  for (int a = 0; a < 16; a++) *reinterpret_cast<unsigned *>(in + (((a << 4) | qt) * 128 + xp * 4)) = as_u32(r[a]);
  __syncthreads();

  // level 2: slots (qt << 4) | b
#pragma unroll
  for (int b = 0; b < 16; b++) r[b] = as_v2(*reinterpret_cast<const unsigned *>(in + (((qt << 4) | b) * 128 + xp * 4)));
  {
    uint4 dv;
    dv.x = lds8_stage<4>(r, qt << 4, xe, syms);
    dv.y = lds8_stage<5>(r, qt << 4, xe, syms);
    dv.z = lds8_stage<6>(r, qt << 4, xe, syms);
    dv.w = lds8_stage<7>(r, qt << 4, xe, syms);
    rb[4 * V224_ROWWORDS] = dv.x; rb[5 * V224_ROWWORDS] = dv.y; rb[6 * V224_ROWWORDS] = dv.z; rb[7 * V224_ROWWORDS] = dv.w;
  }

  // output image [x][q]: rows of 512 B = 32 chunks of 16 B, chunk index XOR (xp & 7)
  v2u16 mnv = r[0];
#pragma unroll
  for (int b = 1; b < 16; b++) mnv = __builtin_elementwise_min(mnv, r[b]);
  {
    uint4 lo0, lo1, hi0, hi1;
    lo0.x = __builtin_amdgcn_perm(as_u32(r[1]), as_u32(r[0]), 0x05040100u);
    lo0.y = __builtin_amdgcn_perm(as_u32(r[3]), as_u32(r[2]), 0x05040100u);
    lo0.z = __builtin_amdgcn_perm(as_u32(r[5]), as_u32(r[4]), 0x05040100u);
    lo0.w = __builtin_amdgcn_perm(as_u32(r[7]), as_u32(r[6]), 0x05040100u);
    lo1.x = __builtin_amdgcn_perm(as_u32(r[9]), as_u32(r[8]), 0x05040100u);
    lo1.y = __builtin_amdgcn_perm(as_u32(r[11]), as_u32(r[10]), 0x05040100u);
    lo1.z = __builtin_amdgcn_perm(as_u32(r[13]), as_u32(r[12]), 0x05040100u);
    lo1.w = __builtin_amdgcn_perm(as_u32(r[15]), as_u32(r[14]), 0x05040100u);
    hi0.x = __builtin_amdgcn_perm(as_u32(r[1]), as_u32(r[0]), 0x07060302u);
    hi0.y = __builtin_amdgcn_perm(as_u32(r[3]), as_u32(r[2]), 0x07060302u);
    hi0.z = __builtin_amdgcn_perm(as_u32(r[5]), as_u32(r[4]), 0x07060302u);
    hi0.w = __builtin_amdgcn_perm(as_u32(r[7]), as_u32(r[6]), 0x07060302u);
    hi1.x = __builtin_amdgcn_perm(as_u32(r[9]), as_u32(r[8]), 0x07060302u);
    hi1.y = __builtin_amdgcn_perm(as_u32(r[11]), as_u32(r[10]), 0x07060302u);
    hi1.z = __builtin_amdgcn_perm(as_u32(r[13]), as_u32(r[12]), 0x07060302u);
    hi1.w = __builtin_amdgcn_perm(as_u32(r[15]), as_u32(r[14]), 0x07060302u);
    const unsigned key = xp & 7;
    unsigned char *row_e = outb + (2 * xp) * 512, *row_o = row_e + 512;
    *reinterpret_cast<uint4 *>(row_e + (((2 * qt) ^ key) * 16)) = lo0;         // q = qt*16 + 0..7
    *reinterpret_cast<uint4 *>(row_e + (((2 * qt + 1) ^ key) * 16)) = lo1;     // q = qt*16 + 8..15
    *reinterpret_cast<uint4 *>(row_o + (((2 * qt) ^ key) * 16)) = hi0;
    *reinterpret_cast<uint4 *>(row_o + (((2 * qt + 1) ^ key) * 16)) = hi1;
  }
  __syncthreads();
  {
    uint4 *dst = reinterpret_cast<uint4 *>(newm + (size_t)ti * 16384);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const unsigned g = i * 512 + th, xl = g >> 5, c = g & 31;
      const uint4 o = *reinterpret_cast<const uint4 *>(outb + xl * 512 + ((c ^ ((xl >> 1) & 7)) * 16));
      dst[g] = o;
    }
  }
  return mnv;
}

// TIN: subtract (minimum of the input - BASE) while loading; TOUT: publish the minimum of the output.
// The port's metrics never decrease, so a launch may skip one of the two: the host alternates
// (TIN,!TOUT) / (!TIN,TOUT) inside a run of launches, the window tolerates two launches of growth.
template <bool TIN, bool TOUT>
__global__ __launch_bounds__(512) void k_acs_lds8(const uint16_t *__restrict__ oldm, uint16_t *__restrict__ newm,
                                                  uint32_t *__restrict__ rows, int row0,
                                                  const uint8_t *__restrict__ syms, V224Dev *ds,
                                                  unsigned pass, uint32_t *rowmeta) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[65536 + 64];
  unsigned *s8 = reinterpret_cast<unsigned *>(lds + 65536);       // 8 + 8 words of reduction scratch
  unsigned char *in = lds, *outb = lds + 32768;
  const unsigned th = threadIdx.x;
  // phase offset between the two workgroups that share a CU (all 512 are resident at once and would
  // otherwise load, compute and store in lockstep): the second half of the grid starts late, so its
  // memory phases fall under the first half's arithmetic and vice versa
  if (blockIdx.x >= gridDim.x / 2) {
#pragma unroll 1
    for (int i = 0; i < LDS8_STAGGER; i++) __builtin_amdgcn_s_sleep(32);      // 32 * 64 cycles each
  }

  // ---- loads: chunk g = i*512 + th (16 B) = row g>>3, 8 states at column (g&7)*8
  const unsigned ti = blockIdx.x;
  uint4 v[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned g = i * 512 + th, q = g >> 3, c = g & 7;
    v[i] = *reinterpret_cast<const uint4 *>(oldm + ((size_t)q << 15) + ti * 64 + c * 8);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) *reinterpret_cast<uint4 *>(in + (i * 512 + th) * 16) = v[i];
  unsigned adj;
  if constexpr (!TIN) { adj = 0; __syncthreads(); }
  else adj = block_min512_in(ds, pass, s8) - V224_BASE;            // contains the barrier after the LDS fill
  const v2u16 adj2 = as_v2((adj & 0xffffu) * 0x10001u);

  const v2u16 mnv = lds8_tile(in, outb, ti, adj2, newm, rows, row0, syms);

  // ---- minimum of what this workgroup wrote ----------------------------------------------------
  if constexpr (!TOUT) {
    if (th == 0 && blockIdx.x == 0) {
      ds->off += (long long)(int)adj;
      for (int t = 0; t < 8; t++) rowmeta[row0 + t] = LDS8_META(t + 1);
    }
  } else {
    unsigned mn = (unsigned)mnv.x < (unsigned)mnv.y ? (unsigned)mnv.x : (unsigned)mnv.y;
    mn = wave_min_u32(mn);
    if ((th & 63) == 0) s8[8 + (th >> 6)] = mn;
    __syncthreads();
    if (th == 0) {
      unsigned m = s8[8];
#pragma unroll
      for (int w = 1; w < 8; w++) m = s8[8 + w] < m ? s8[8 + w] : m;
      ds->blkmin[(pass + 1) & 1][blockIdx.x] = m;
      if (blockIdx.x == 0) {
        ds->nmin[(pass + 1) & 1] = gridDim.x;
        ds->off += (long long)(int)adj;             // native port branch metrics: nothing dropped
        for (int t = 0; t < 8; t++) rowmeta[row0 + t] = LDS8_META(t + 1);
      }
    }
  }
}

// decision for NEW state s of the row written by stage tau (1..8) of an LDS pass; r = that row's base
__device__ __forceinline__ unsigned lds8_get_decision(const uint32_t *__restrict__ r, unsigned tau, unsigned s) {
  const unsigned x = (s >> tau) & 0x7fffu;
  const unsigned qout = ((s & ((1u << tau) - 1u)) << (8 - tau)) | (s >> (15 + tau));
  const unsigned ti = x >> 6, xl = x & 63u, xp = xl >> 1, h = xl & 1u;
  const unsigned lb = 3u - ((tau - 1u) & 3u);
  unsigned th, slot;
  if (tau <= 4) { th = ((qout & 15u) << 5) | xp; slot = qout >> 4; }
  else          { th = ((qout >> 4) << 5) | xp;  slot = qout & 15u; }
  // insert order inside a stage: butterfly BF = slot with bit lb squeezed out, low slot first
  const unsigned bf = ((slot >> (lb + 1)) << lb) | (slot & ((1u << lb) - 1u));
  const unsigned bit = 16u * h + 2u * bf + ((slot >> lb) & 1u);
  return ((r[ti * 512u + th] >> bit) & 1u) ^ 1u;                  // rows hold NOT(decision)
}
