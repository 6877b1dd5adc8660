// v224_lds15.hip.inc -- LDS-staged four-level ACS pass: 15 trellis steps per launch (engine LDS15).
//
// Same in-place butterfly network as v224_fused.hip.inc / v224_lds.hip.inc, with K = 15 (XB = 8):
// a workgroup owns ALL 2^15 slots q of one x (x = the low 8 state bits = blockIdx.x), 64 KiB of
// metrics, so the kernel boundary, the minimum bookkeeping and the HBM round trip of the metrics are
// paid once per 15 steps instead of once per 8.  Index algebra checked on the CPU against the oracle
// by scratch/l15_model.py.
//
// Metric layout "L15" in HBM (both buffers, only while this engine runs; see k_l15_from_nat/to_nat):
//      phys(s) = (s >> 15) << 15 | (s & 0xff) << 7 | (s >> 8) & 0x7f
// A tile's OUTPUT (new states s' = x << 15 | q) is then one contiguous 64 KiB block, row q & 0xff, column q >> 8,
// and its INPUT 256 runs of 256 B, one from every tile of the previous pass.  (With the natural layout the reads
// would be 2-byte gathers: old[(q << 8) + x].)
//
// 1024 threads x 16 packed VGPRs (two slots per VGPR) = 32 768 slots.  Four register levels with the tile in LDS
// between them (each exchange: 16 ds_write_b32 in place, barrier, 16 ds_read_b32 / 4 ds_read_b128):
//      level 0  steps  1-4   pair slot bits 14..11   reg = bits 14..11, packed over bit 0, thread = bits 10..1
//      level 1  steps  5-8   pair slot bits 10..7    reg = bits 10..7,  packed over bit 0, thread = 14..11 | 6..1
//      level 2  steps  9-12  pair slot bits  6..3    reg = bits  6..3,  packed over bit 0, thread = 14..7 | 2..1
//      level 3  steps 13-15  pair slot bits  2..0    reg = bits 9,2,1,0, packed over bit 8 (16 v_perm re-pair),
//                                                    wave = 6..3, lanes = 14..11 | 10 | 7
// Level 0 takes its operands straight from HBM: register a of a wave is one whole 256-byte run.  Level 3 maps lanes to
// output columns: a packed register is two neighbouring columns, the 64 lanes of a wave hold two complete 256-byte
// output rows per register pair, and the rows go straight from registers to HBM (8 global_store_dwordx2 per thread).
// So the LDS holds only the in-place tile (70 KiB: two workgroups, of two decoders, fit a CU), there are three
// barriers, and PMC reports no bank conflict: the image is padded by 4 dwords per 64 and 8 per 1024 (dword d sits at
// d + (d >> 6) * 4 + (d >> 10) * 8), which keeps every per-register offset an immediate.
//
// Decisions: one dword per thread and stage, word index x * 1024 + thread, bit 8*(2*which output + half) +
// butterfly; rows hold NOT(decision) as in the other packed engines.  A pass may wrap the ring.
#pragma once

// waves w, w + 4, w + 8, w + 12 of a workgroup share a SIMD: priorities 3, 2, 1, 0 (s_setprio takes an immediate)
__device__ __forceinline__ void l15_stagger_prio(unsigned th) {
  const unsigned rank = (unsigned)__builtin_amdgcn_readfirstlane((int)(th >> 8));
  if (rank == 0) __builtin_amdgcn_s_setprio(3);
  else if (rank == 1) __builtin_amdgcn_s_setprio(2);
  else if (rank == 2) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
#define LDS15_META(tau) ((1u << 17) | (15u << 8) | (unsigned)(tau))
// input image: dword d sits at d + (d >> 6) * 4 + (d >> 10) * 8 (the level-3 lanes differ in d bits 10..13 and would
// otherwise fall on the same banks)
#define L15_PADA       1096u                  // dwords per 1024-dword slab
#define L15_IN_BYTES   70144u                 // (16384 + 1024 + 128) dwords
#define L15_LDS_BYTES  70272u                 // the image + 128 bytes of reduction scratch
// The input normalisation (subtract the previous launch's minimum - BASE) is folded into stage 5's constants, not
// stage 1's: the minima's load, wave reduction and LDS hand-over then have the whole of level 0 to finish and share
// the barrier of the first tile exchange.
#define L15_ADJ_STAGE  4

__host__ __device__ constexpr int l15_qpos(int j, int t) { return j >= 15 - t ? j - (15 - t) : j + t + 8; }
__host__ __device__ constexpr unsigned l15_qmask(int t) {
  unsigned m = 0;
  for (int j = 0; j < 15; j++)
    if (j != 14 - t && ((V224_P1H >> l15_qpos(j, t)) & 1u)) m |= 1u << j;
  return m;
}
__host__ __device__ constexpr int l15_level(int t) { return t < 12 ? t / 4 : 3; }
__host__ __device__ constexpr int l15_lb(int t) { return t < 12 ? 3 - (t % 4) : 14 - t; }      // register-index bit paired
__host__ __device__ constexpr unsigned l15_regslot(int level, unsigned a) {                    // register index as slot bits
  return level == 0 ? a << 11 : level == 1 ? a << 7 : level == 2 ? a << 3 : (((a >> 3) << 9) | (a & 7u));
}
__host__ __device__ constexpr int l15_packbit(int level) { return level == 3 ? 8 : 0; }

template <int T, int BF>
__device__ __forceinline__ void l15_bfly(v2u16 (&r)[16], unsigned &acc, const v2u16 K0, const v2u16 K1) {
  constexpr int LEVEL = l15_level(T), lb = l15_lb(T);
  constexpr unsigned rq = (((unsigned)BF >> lb) << (lb + 1)) | ((unsigned)BF & ((1u << lb) - 1u));
  constexpr unsigned rj = rq | (1u << lb);
  constexpr unsigned qreg = l15_regslot(LEVEL, rq);
  constexpr unsigned sgn = cpar(qreg & l15_qmask(T));
  constexpr unsigned kh = (l15_qmask(T) >> l15_packbit(LEVEL)) & 1u;   // the high half's parity differs from the low half's
  // i & 1 of the MSB-clear predecessor = slot bit 15-T (T >= 1): static when that bit is a register bit
  constexpr unsigned ibit = T >= 1 ? (1u << (15 - T)) : 0u;
  constexpr bool i0_static = (l15_regslot(LEVEL, 15u) & ibit) != 0u;
  constexpr unsigned i0 = i0_static ? ((qreg & ibit) ? 1u : 0u) : 0u;
  // K = the thread's pair of branch metrics: half j holds bm for (thread parity ^ j) even, i.e. c for half 0 in a thread
  // of even parity.  This butterfly's own parity bit `sgn` and the packing bit `kh` only pick HALVES of K -- op_sel
  // modifiers of the packed add, no instruction: cc = bm of the even-parity branch for this slot, cn = 510 - cc.
  const v2u16 K = i0 ? K1 : K0;
  const v2u16 cc = __builtin_shufflevector(K, K, (int)sgn, (int)(sgn ^ kh));
  const v2u16 cn = __builtin_shufflevector(K, K, (int)(sgn ^ 1u), (int)(sgn ^ kh ^ 1u));
  const v2u16 oi = r[rq], oj = r[rj];
  const v2u16 Av = oi + cc, Bv = oj + cn, Cv = oi + cn, Dv = oj + cc;
  const unsigned d0 = as_u32(Av - Bv), d1 = as_u32(Cv - Dv);       // bit 15 / 31 = (A < B) = NOT decision
  r[rq] = __builtin_elementwise_min(Av, Bv);
  r[rj] = __builtin_elementwise_min(Cv, Dv);
  // The four sign bits sit at bit 7 of bytes 1 and 3 of d0, d1.  Selectors 8 .. 11 of v_perm_b32 replicate the sign bit
  // of bytes 1, 3, 5, 7 of {d1, d0} over a whole byte: P holds the four decisions as 0x00 / 0xff, byte 2*which + half.
  // Butterfly 0 fills all eight bits of every byte with its decision; butterfly k overwrites bit k under a mask
  // (v_bfi): 2 instructions per butterfly.
  const unsigned P = __builtin_amdgcn_perm(d1, d0, 0x0b0a0908u);
  if constexpr (BF == 0) acc = P;
  else asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(acc) : "s"(0x01010101u << BF), "v"(P), "v"(acc));
}

template <int T, int... BF>
__device__ __forceinline__ void l15_bflies(v2u16 (&r)[16], unsigned &acc, const v2u16 K0, const v2u16 K1,
                                           std::integer_sequence<int, BF...>) {
  (l15_bfly<T, BF>(r, acc, K0, K1), ...);
}

// The 30 symbols of a pass, fetched with scalar loads: 9 aligned dwords starting at the dword that holds
// syms[0] (the pointer itself may have any alignment); W[8] is only read when it holds one of the 30 bytes.
struct L15Syms { unsigned w0, w1, w2, w3, w4, w5, w6, w7, w8, sh; };
__device__ __forceinline__ L15Syms l15_load_syms(const uint8_t *__restrict__ syms) {
  const unsigned mis = (unsigned)((uintptr_t)syms & 3u);
  const unsigned *__restrict__ w = reinterpret_cast<const unsigned *>(syms - mis);     // still a global pointer
  L15Syms y;
  y.w0 = w[0]; y.w1 = w[1]; y.w2 = w[2]; y.w3 = w[3]; y.w4 = w[4]; y.w5 = w[5]; y.w6 = w[6]; y.w7 = w[7];
  unsigned last = 0u;
  if (mis == 3u) last = w[8];
  y.w8 = last;
  y.sh = mis * 8u;
  return y;
}
template <int I> __device__ __forceinline__ unsigned l15_symword(const L15Syms &y) {
  if constexpr (I == 0) return y.w0; else if constexpr (I == 1) return y.w1; else if constexpr (I == 2) return y.w2;
  else if constexpr (I == 3) return y.w3; else if constexpr (I == 4) return y.w4; else if constexpr (I == 5) return y.w5;
  else if constexpr (I == 6) return y.w6; else if constexpr (I == 7) return y.w7; else return y.w8;
}
template <int KB>
__device__ __forceinline__ unsigned l15_sym(const L15Syms &y) {
  // a byte never straddles two words; written without a 64-bit combine (which would keep the words in memory)
  const unsigned pos = y.sh + 8u * (KB & 3);
  const unsigned wsel = (pos & 32u) ? l15_symword<(KB >> 2) + 1>(y) : l15_symword<(KB >> 2)>(y);
  return (wsel >> (pos & 31u)) & 0xffu;
}

// Per-thread parities of all 15 stages, looked up instead of counted: word [level][thread], field k (bits 5k .. 5k+4) =
// 16 * parity(qthr(level, thread) & qmask(4 level + k)).  Filled once per process by l15_fill_rot_tab() (host, from the same
// constexpr index algebra the kernel uses); 16 KiB, L2-resident; a thread fetches its four words while its metrics load.
__device__ unsigned l15_rot_tab[4 * 1024];
__host__ __device__ constexpr unsigned l15_qthr(int level, unsigned th) {
  return level == 0 ? th << 1
       : level == 1 ? ((th >> 6) << 11) | ((th & 63u) << 1)
       : level == 2 ? ((th >> 2) << 7) | ((th & 3u) << 1)
       : ((((th >> 2) & 15u) << 11) | (((th >> 1) & 1u) << 10) | ((th & 1u) << 7) | ((th >> 6) << 3));
}
static void l15_build_rot_tab(unsigned *tab) {
  for (int level = 0; level < 4; level++)
    for (unsigned th = 0; th < 1024; th++) {
      unsigned w = 0;
      for (int k = 0; k < 4 && 4 * level + k < 15; k++) {
        const unsigned v = l15_qthr(level, th) & l15_qmask(4 * level + k);
        w |= (cpar(v) << 4) << (5 * k);
      }
      tab[level * 1024 + th] = w;
    }
}

// one trellis step on the 32 slots a thread holds; qthr = the thread's own slot bits (in place).
// Everything that depends only on the symbols and on x is wave-uniform (SALU): the pair (c, 510 - c) packed into one
// scalar.  Per thread only the parity of its slot bits matters -- it swaps the two: ONE rotate (v_alignbit by 0 or 16)
// per pair; everything else a butterfly needs from it is a choice of halves (see l15_bfly).
template <int T>
__device__ __forceinline__ unsigned l15_stage(v2u16 (&r)[16], const unsigned qthr, const unsigned x,
                                              const L15Syms &y, const unsigned adj, const unsigned rotw) {
  const unsigned s0 = l15_sym<2 * T>(y), s1 = l15_sym<2 * T + 1>(y);
  const unsigned c0 = s0 + 255u - s1, c1 = s0 + s1;            // port.c:170 for i even / odd
  constexpr unsigned xmask = (V224_P1H >> T) & 0xffu;
  // parity of the thread's part of the state number: looked up, not counted -- rotw = the thread's word of l15_rot_tab for
  // this level, field k (5 bits) = 16 * parity(qthr & qmask(4 level + k)); v_alignbit uses bits 4..0 of its shift: 0 or 16
  const unsigned rot = (T & 3) ? rotw >> (5 * (T & 3)) : rotw;
  // scalar pairs: half 0 = bm for even parity, half 1 = 510 - bm; stage 5 also carries the input normalisation; the
  // tile's own parity (x is uniform) swaps the halves on the scalar side
  const unsigned a16 = (T == L15_ADJ_STAGE) ? adj : 0u;
  const unsigned px = (unsigned)__popc(x & xmask) & 1u;
  const unsigned e0 = px ? 510u - c0 : c0, e1 = px ? 510u - c1 : c1;           // (a select of c / 510 - c, not a rotate: stays SALU)
  const unsigned P0 = ((e0 - a16) & 0xffffu) | ((510u - e0 - a16) << 16);
  const unsigned P1 = ((e1 - a16) & 0xffffu) | ((510u - e1 - a16) << 16);
  v2u16 K0, K1;
  if constexpr (T == 0) {                                        // i & 1 = x & 1: uniform
    const unsigned Pu = (x & 1u) ? P1 : P0;
    K0 = as_v2(__builtin_amdgcn_alignbit(Pu, Pu, rot)); K1 = K0;
  } else if constexpr (T == 4 || T == 8 || T == 12) {            // i & 1 is a thread bit
    const unsigned Ms = (unsigned)((int)(qthr << (31 - (15 - T))) >> 31);
    const unsigned Pt = P0 ^ (Ms & (P0 ^ P1));
    K0 = as_v2(__builtin_amdgcn_alignbit(Pt, Pt, rot)); K1 = K0;
  } else {
    K0 = as_v2(__builtin_amdgcn_alignbit(P0, P0, rot));
    K1 = as_v2(__builtin_amdgcn_alignbit(P1, P1, rot));
  }
  unsigned acc = 0;
  l15_bflies<T>(r, acc, K0, K1, std::make_integer_sequence<int, 8>{});
  return acc;
}

// decision rows are written once and read back only by the traceback: nontemporal
__device__ __forceinline__ void l15_dstore(uint32_t *p, unsigned v) { __builtin_nontemporal_store(v, p); }

// NOARITH: the placement probe's build (place_metrics): the same loads, LDS traffic and stores, no trellis arithmetic
template <bool NOARITH, bool TIN, bool TOUT>
__global__ __launch_bounds__(1024) void k_acs_lds15(const uint16_t *__restrict__ oldm, uint16_t *__restrict__ newm,
                                                    uint32_t *__restrict__ rows, int row0, int len,
                                                    const uint8_t *__restrict__ syms, V224Dev *ds,
                                                    unsigned pass, uint32_t *rowmeta) {
  extern __shared__ __attribute__((aligned(16))) unsigned char l15_lds[];
  unsigned char *in = l15_lds;
  unsigned *s16 = reinterpret_cast<unsigned *>(l15_lds + L15_LDS_BYTES - 128u);           // 16 + 16 words
  const unsigned th = threadIdx.x, x = blockIdx.x;
  const L15Syms sy = l15_load_syms(syms);          // before any store of this kernel: scalar loads
  const unsigned rw0 = l15_rot_tab[th], rw1 = l15_rot_tab[1024 + th], rw2 = l15_rot_tab[2048 + th], rw3 = l15_rot_tab[3072 + th];

  v2u16 r[16], mnv;
  // The previous launch's per-workgroup minima go FIRST into the memory pipeline (vector loads return in order): their
  // reduction and its barrier then run while the sixteen metric loads behind them are still in flight, instead of after
  // them.  asm, because the compiler would wait for this load with vmcnt(0) -- i.e. for the metric loads as well.
  unsigned mpre = 0xffffffffu, nmin_v = 0u;
  if constexpr (TIN) {
    // entry th of the writer's minima (1 .. 512 of them, one per workgroup; the array holds 4 096 words, so the load is in
    // bounds whatever their number) AND their number, both at once: fetching the number first and then entry
    // min(th, n - 1) put a whole memory round trip in front of the metric loads.  Entries beyond the number are dropped below.
    const unsigned *a = ds->blkmin[pass & 1];
    const unsigned *np = &ds->nmin[pass & 1];
    asm volatile("global_load_dword %0, %1, %2" : "=v"(mpre) : "v"(th << 2), "s"(a) : "memory");
    asm volatile("global_load_dword %0, %1, %2" : "=v"(nmin_v) : "v"(0u), "s"(np) : "memory");
  }
  // ---- level 0 operands straight from HBM: register a of thread th is dword (th & 63) of run (a << 4 | th >> 6),
  //      the 256 bytes that tile (a << 4 | th >> 6) of the previous pass wrote for this x
  {
    // uniform base (tile x, run a) in SGPRs + ONE 32-bit per-thread byte offset: global_load_dword vdst, voff, s[base].
    // Written as asm because the compiler folds base and offset into sixteen 64-bit VGPR addresses otherwise (30 VALU
    // instructions and 30 VGPRs).  The loads are waited for below (the compiler does not count them).  One wait for all
    // sixteen, not one per butterfly of stage 1: see DESIGN.md section 8, "lock-step".
    const unsigned char *base = reinterpret_cast<const unsigned char *>(oldm) + ((size_t)x << 8);
    const unsigned voff = ((th >> 6) << 16) | ((th & 63u) << 2);
#pragma unroll
    for (int a = 0; a < 16; a++) {                                             // run + 16: 16 x 32768 u16 = 2^20 bytes
      unsigned v;
      asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(voff), "s"(base + ((size_t)a << 20)) : "memory");
      r[a] = as_v2(v);
    }
  }
  // Uniform offsets do not enter any decision (only differences do), and four more steps of growth (4 x 510) stay inside
  // the u16 window: 4096 + 12 730 + 15 x 510 of an un-adjusted predecessor + 2 040 = 26 516 < 2^15.  So level 0 runs on
  // the metrics as they are; the wave minima wait in LDS behind the barrier of the first tile exchange.
  unsigned adj = 0;
  if constexpr (TIN) {
    asm volatile("s_waitcnt vmcnt(16)" : "+v"(mpre), "+v"(nmin_v));  // the minima have landed (the 16 loads behind them may not have)
    unsigned m = wave_min_u32(th < nmin_v ? mpre : 0xffffffffu);
    if ((th & 63u) == 0) s16[th >> 6] = m;
  }
  // the sixteen asm loads above have landed after this (ties the registers to the wait so that no use moves above it)
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]),
                 "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
               :: "memory");
  // decision rows of the 15 stages (the pass may wrap the ring): uniform row base + per-thread word
  const unsigned woffb = (x * 1024u + th) * 4u;            // 32-bit byte offset: uniform base + per-lane offset addressing
#define L15_ROW(t) reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(rows + (size_t)((row0 + (t)) >= len ? row0 + (t) - len : row0 + (t)) * V224_ROWWORDS) + woffb)
#define L15_STAGES4(T0, QTHR, RW)                                                                  \
  {                                                                                                \
    const unsigned d0_ = l15_stage<T0>(r, QTHR, x, sy, adj, RW), d1_ = l15_stage<T0 + 1>(r, QTHR, x, sy, adj, RW); \
    const unsigned d2_ = l15_stage<T0 + 2>(r, QTHR, x, sy, adj, RW), d3_ = l15_stage<T0 + 3>(r, QTHR, x, sy, adj, RW); \
    l15_dstore(L15_ROW(T0), d0_); l15_dstore(L15_ROW(T0 + 1), d1_); l15_dstore(L15_ROW(T0 + 2), d2_); l15_dstore(L15_ROW(T0 + 3), d3_); \
  }

  // ---- level 0: slots a << 11 | th << 1 | h ; dword a << 10 | th
  {
    unsigned char *p = in + (th + (th >> 6) * 4u) * 4u;
    if constexpr (!NOARITH) L15_STAGES4(0, th << 1, rw0)
#pragma unroll
    for (int a = 0; a < 16; a++) *reinterpret_cast<unsigned *>(p + a * (L15_PADA * 4)) = as_u32(r[a]);
  }
  __syncthreads();
  if constexpr (TIN) {                  // the previous launch's minimum, handed over in LDS before the barrier above
    unsigned q = s16[0];
#pragma unroll
    for (int w = 1; w < 16; w++) q = s16[w] < q ? s16[w] : q;
    adj = q - V224_BASE;
  }
  // ---- level 1: slots hi4 << 11 | a << 7 | lo6 << 1 | h ; dword hi4 << 10 | a << 6 | lo6
  {
    const unsigned hi4 = th >> 6, lo6 = th & 63u;
    unsigned char *p = in + hi4 * (L15_PADA * 4u) + lo6 * 4u;
#pragma unroll
    for (int a = 0; a < 16; a++) r[a] = as_v2(*reinterpret_cast<const unsigned *>(p + a * 272));
    if constexpr (!NOARITH) L15_STAGES4(4, (hi4 << 11) | (lo6 << 1), rw1)
#pragma unroll
    for (int a = 0; a < 16; a++) *reinterpret_cast<unsigned *>(p + a * 272) = as_u32(r[a]);
  }
  __syncthreads();
  // ---- level 2: slots hi8 << 7 | a << 3 | lo2 << 1 | h ; dword hi8 << 6 | a << 2 | lo2
  {
    const unsigned hi8 = th >> 2, lo2 = th & 3u;
    unsigned char *p = in + hi8 * 272u + (hi8 >> 4) * 32u + lo2 * 4u;
#pragma unroll
    for (int a = 0; a < 16; a++) r[a] = as_v2(*reinterpret_cast<const unsigned *>(p + a * 16));
    if constexpr (!NOARITH) L15_STAGES4(8, (hi8 << 7) | (lo2 << 1), rw2)
#pragma unroll
    for (int a = 0; a < 16; a++) *reinterpret_cast<unsigned *>(p + a * 16) = as_u32(r[a]);
  }
  __syncthreads();
  // level 3 has no barrier behind it: staggered priorities let the first wave's metric stores leave while the others
  // still compute.  That is what makes two decoders' launch chains pair well: DESIGN.md section 8, "lock-step".
  l15_stagger_prio(th);
  // ---- level 3: wave = t63 (slots 6..3), lanes = t14 (slots 14..11) | t10 | t7: for one register the 64 lanes hold
  //      two complete output rows (row = slots 7..0, 128 columns = slots 14..8); register a = b9:b2:b1:b0, packed over
  //      slot bit 8
  {
    const unsigned t63 = th >> 6, t14 = (th >> 2) & 15u, t10 = (th >> 1) & 1u, t7 = th & 1u;
    const unsigned char *p = in + (t14 * L15_PADA + t10 * 544u + t7 * 68u + t63 * 4u) * 4u;
    uint4 D[2][2];
#pragma unroll
    for (int b9 = 0; b9 < 2; b9++)
#pragma unroll
      for (int b8 = 0; b8 < 2; b8++) D[b9][b8] = *reinterpret_cast<const uint4 *>(p + b9 * 1088 + b8 * 544);
#pragma unroll
    for (int b9 = 0; b9 < 2; b9++) {
      const unsigned lo[4] = {D[b9][0].x, D[b9][0].y, D[b9][0].z, D[b9][0].w};
      const unsigned hi[4] = {D[b9][1].x, D[b9][1].y, D[b9][1].z, D[b9][1].w};
#pragma unroll
      for (int w = 0; w < 4; w++) {
        r[b9 * 8 + w * 2 + 0] = as_v2(__builtin_amdgcn_perm(hi[w], lo[w], 0x05040100u));
        r[b9 * 8 + w * 2 + 1] = as_v2(__builtin_amdgcn_perm(hi[w], lo[w], 0x07060302u));
      }
    }
    const unsigned qthr = (t14 << 11) | (t10 << 10) | (t7 << 7) | (t63 << 3);
    if constexpr (!NOARITH) {
      const unsigned d0_ = l15_stage<12>(r, qthr, x, sy, adj, rw3), d1_ = l15_stage<13>(r, qthr, x, sy, adj, rw3);
      const unsigned d2_ = l15_stage<14>(r, qthr, x, sy, adj, rw3);
      l15_dstore(L15_ROW(12), d0_); l15_dstore(L15_ROW(13), d1_); l15_dstore(L15_ROW(14), d2_);
    }
    v2u16 mnv_ = r[0];
#pragma unroll
    for (int b = 1; b < 16; b++) mnv_ = __builtin_elementwise_min(mnv_, r[b]);
    mnv = mnv_;
    const unsigned rowb = (t7 << 7) | (t63 << 3);
    // rows straight to HBM: row rowb + low3 of this tile's 64 KiB block, 8 bytes at column t14 << 3 | t10 << 2
    // (32 lanes x 8 B = the 256 bytes of the row; the other 32 lanes write row + 128)
    unsigned char *o = reinterpret_cast<unsigned char *>(newm + (size_t)x * 32768u) + rowb * 256u + ((t14 << 3) | (t10 << 2)) * 2u;
#pragma unroll
    for (int l3 = 0; l3 < 8; l3++) {
      uint2 w; w.x = as_u32(r[l3]); w.y = as_u32(r[8 + l3]);
      *reinterpret_cast<uint2 *>(o + l3 * 256) = w;
    }
  }
#undef L15_STAGES4
#undef L15_ROW

  // ---- minimum of what this workgroup wrote, running offset, row layout codes
  if constexpr (TOUT) {
    unsigned mn = (unsigned)mnv.x < (unsigned)mnv.y ? (unsigned)mnv.x : (unsigned)mnv.y;
    mn = wave_min_u32(mn);
    if ((th & 63) == 0) s16[16 + (th >> 6)] = mn;
    __syncthreads();
    if (th == 0) {
      unsigned m = s16[16];
#pragma unroll
      for (int w = 1; w < 16; w++) m = s16[16 + w] < m ? s16[16 + w] : m;
      ds->blkmin[(pass + 1) & 1][x] = m;
      if (x == 0) ds->nmin[(pass + 1) & 1] = gridDim.x;
    }
  }
  if (th == 0 && x == 0) {
    ds->off += (long long)(int)adj;
    for (int t = 0; t < 15; t++) { int rr = row0 + t; if (rr >= len) rr -= len; rowmeta[rr] = LDS15_META(t + 1); }
  }
}

// decision for NEW state s of the row written by stage tau (1..15) of an LDS15 pass; r = that row's base
__device__ __forceinline__ unsigned lds15_get_decision(const uint32_t *__restrict__ r, unsigned tau, unsigned s) {
  const unsigned x = (s >> tau) & 0xffu;
  const unsigned q = ((s & ((1u << tau) - 1u)) << (15u - tau)) | (s >> (tau + 8u));
  const unsigned t = tau - 1u;
  unsigned th, a, h, lb;
  if (t < 4)       { th = (q >> 1) & 1023u;                       a = q >> 11;        h = q & 1u; lb = 3u - t; }
  else if (t < 8)  { th = ((q >> 11) << 6) | ((q >> 1) & 63u);    a = (q >> 7) & 15u; h = q & 1u; lb = 7u - t; }
  else if (t < 12) { th = ((q >> 7) << 2) | ((q >> 1) & 3u);      a = (q >> 3) & 15u; h = q & 1u; lb = 11u - t; }
  else {
    th = (((q >> 3) & 15u) << 6) | ((q >> 11) << 2) | (((q >> 10) & 1u) << 1) | ((q >> 7) & 1u);
    a = (((q >> 9) & 1u) << 3) | (q & 7u); h = (q >> 8) & 1u; lb = 14u - t;
  }
  const unsigned bf = ((a >> (lb + 1u)) << lb) | (a & ((1u << lb) - 1u));
  const unsigned bit = 8u * (2u * ((a >> lb) & 1u) + h) + bf;
  return ((r[x * 1024u + th] >> bit) & 1u) ^ 1u;                  // rows hold NOT(decision)
}

// ---- layout conversion: natural <-> L15 ------------------------------------------------------------
// Workgroup (h, mh): natural states s = h << 15 | (mh*64 + m) << 8 | l  (32 KiB contiguous), L15 position
// h << 15 | l << 7 | mh*64 + m  (256 runs of 128 B).  Transposed through LDS, rows padded by one dword.
__global__ __launch_bounds__(512) void k_l15_from_nat(const uint16_t *__restrict__ nat, uint16_t *__restrict__ l15) {
  __shared__ uint16_t t[64 * 258];
  const unsigned th = threadIdx.x, h = blockIdx.x >> 1, mh = blockIdx.x & 1u;
  const unsigned *src = reinterpret_cast<const unsigned *>(nat + ((size_t)h << 15) + ((size_t)mh << 14));
#pragma unroll 4
  for (int i = 0; i < 16; i++) {                     // dword g: m = g >> 7, l pair = g & 127
    const unsigned g = i * 512 + th, m = g >> 7, lp = g & 127u;
    *reinterpret_cast<unsigned *>(&t[m * 258 + 2 * lp]) = src[g];
  }
  __syncthreads();
#pragma unroll 4
  for (int i = 0; i < 16; i++) {                     // dword g: l = g >> 5, m pair = g & 31
    const unsigned g = i * 512 + th, l = g >> 5, mp = g & 31u;
    const unsigned v = (unsigned)t[(2 * mp) * 258 + l] | ((unsigned)t[(2 * mp + 1) * 258 + l] << 16);
    reinterpret_cast<unsigned *>(l15 + ((size_t)h << 15) + (l << 7) + (mh << 6))[mp] = v;
  }
}
__global__ __launch_bounds__(512) void k_l15_to_nat(const uint16_t *__restrict__ l15, uint16_t *__restrict__ nat) {
  __shared__ uint16_t t[64 * 258];
  const unsigned th = threadIdx.x, h = blockIdx.x >> 1, mh = blockIdx.x & 1u;
#pragma unroll 4
  for (int i = 0; i < 16; i++) {
    const unsigned g = i * 512 + th, l = g >> 5, mp = g & 31u;
    const unsigned v = reinterpret_cast<const unsigned *>(l15 + ((size_t)h << 15) + (l << 7) + (mh << 6))[mp];
    t[(2 * mp) * 258 + l] = (uint16_t)v;
    t[(2 * mp + 1) * 258 + l] = (uint16_t)(v >> 16);
  }
  __syncthreads();
  unsigned *dst = reinterpret_cast<unsigned *>(nat + ((size_t)h << 15) + ((size_t)mh << 14));
#pragma unroll 4
  for (int i = 0; i < 16; i++) {
    const unsigned g = i * 512 + th, m = g >> 7, lp = g & 127u;
    dst[g] = *reinterpret_cast<const unsigned *>(&t[m * 258 + 2 * lp]);
  }
}
__host__ __device__ constexpr unsigned l15_phys(unsigned s) {
  return ((s >> 15) << 15) | ((s & 0xffu) << 7) | ((s >> 8) & 0x7fu);
}
