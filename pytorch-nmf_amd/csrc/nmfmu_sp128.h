// Software-pipelined, one-wave-per-SIMD form of the fused beta = 1 MU half-step at padded rank 128 with 64 owner rows
// per wave (two 32-row groups): the structure of nmfmu_sp.h on the ping-pong kernel's 256-row tiles.
//
// Same mathematics, HBM layouts (256-row X tiles in fragment order, one 4 KiB piece per 32 owner rows) and epilogues as
// nmfmu::pp_kernel<128, f16, kModeMU> (nmfmu_pp.h), and the same MFMA order per accumulator: rank steps ascending in
// GEMM1, (tt, m2) ascending within a tile and tiles ascending in GEMM2 -- bit-identical factors at equal contraction
// splits.  A workgroup is FOUR waves; wave w owns the rows of the ping-pong kernel's waves 2 w and 2 w + 1 (owner group
// og = 0 / 1), so every panel operand read feeds two MFMAs:
//
//   phase A(t): 32 MFMAs of GEMM1(t+1) -> S[(t+1) & 1][og]     fillers: their 16 ds_read_b128 and the VALU of tile t's
//                                                              ratio stage (S[t & 1], X(t) -> packed fp16 ratios gn)
//               s_waitcnt vmcnt(8); s_barrier                  (panel tile t+2 has landed and is visible to every wave)
//   phase B(t): 32 MFMAs of GEMM2(t) (acc[og] += gn[og] x P1^T) fillers: their 32 ds_read_b64_tr_b16 (gathers from the
//                                                              row-major slot, FusedCfg::TR), the LDS-DMA of panel tile
//                                                              t+3 (4 pieces per wave), the 8 X loads of tile t+2
//               s_waitcnt vmcnt(12)                            (X(t+1) has landed)
//
// Where the ratio stage's VALU sits is a template parameter (RB, below): the shipped instance runs RB of tile t+1's 64
// reciprocals per lane in the gaps of phase B(t) and spreads the rest of the stage over phase A(t+1) by issue cost.
//
// The panel ring has four 16 KiB slots = 64 KiB: every operand is base register + 16-bit immediate (as nmfmu_sp2.h).
// Register plan: accumulators (2 x 4 x 16 = 128) and owner fragments (2 x 8 x 4 = 64) in AGPRs; two S tiles (2 x 64), the
// ratios (32), the eps seed tile (16), X (2 x 32), the operand rings and 24 LDS address registers in VGPRs (hipcc lets
// the GEMM1 and GEMM2 rings share registers: 256 VGPR + 192 AGPR, no scratch; tests/test_sp128_layout.py reads the report).
#pragma once
#include "nmfmu_sp.h"

namespace nmfmu {

template <int OPT>
struct SP128Cfg {
  static constexpr int R_PAD = 128;
  static constexpr int BM = 256, WAVES = 4, THREADS = 256;
  static constexpr int KS = R_PAD / 16, RT = R_PAD / 32, ROWB = 2 * R_PAD, IMG = kBK * ROWB;
  static constexpr int NSLOT = 4, PF = 4;
  static constexpr int N1 = 2 * KS, N2 = 4 * RT;          // stream entries of GEMM1 / GEMM2 per tile: TWO MFMAs each
  static constexpr int NPW = IMG / 1024 / WAVES;          // LDS-DMA pieces per wave and tile
  static constexpr int XTILE = BM * kBK * 2;              // one X tile: 256 rows x 64 columns x 2 bytes
  static constexpr int GOPS = 10;                         // VALU instructions per group of four elements
  static constexpr int NEL = 16 * GOPS;                   // ... of one tile's ratio stage
  static constexpr int LDS_MAIN = NSLOT * IMG;
  static constexpr int LDS_EPI = 2 * WAVES * 32 * R_PAD * 4;   // fused-apply staging tile per 32-row group
  static constexpr int LDS_BYTES = LDS_MAIN > LDS_EPI ? LDS_MAIN : LDS_EPI;
  static_assert(OPT == kOpF16, "fp16 operands");
  static_assert(N1 == 16 && N2 == 16 && NPW == 4 && NSLOT * IMG <= 65536, "schedule tables below; every LDS offset an immediate");
};

// ---- placement of the ratio stage (template parameter RB of sp128_kernel; tests/test_sp128_respace.py replays these tables).
// RB = 0 is the schedule above: all of tile t's ratio stage in phase A(t), five instructions per MFMA gap.  RB > 0 moves the
// first RB reciprocals of tile t+1 into the MFMA gaps of phase B(t) -- S(t+1) is complete when phase A(t) ends and nothing
// writes its buffer before GEMM1(t+3) -- and re-spaces what stays in phase A by issue cost (transcendental = 2 plain).  Every
// instruction works in place on the S register: reciprocal, multiply by the fp16 half of the X word, then the pack reads two.
//
// Units of four elements are taken in the order their S tiles complete: unit u = (tt = u >> 3, og = (u >> 2) & 1, d-pair
// u & 3); element x = 4 u + pos, pack y = 2 u + h.
// hipcc pads (s_nop 0) in front of an asm statement that touches a register an earlier asm statement wrote unless one of its
// OWN instructions -- scalar upkeep, or a pad it has already placed -- lies between the two: asm statements count as no wait
// state.  The MFMA chains (S: every second entry, accumulators and operand ring: every fourth) owe such a pad about every
// second entry; with hipcc's scalar code kept at the seam in front of an entry's first MFMA those pads fall behind the
// counted wait.  A ratio-stage consumer kSP128Dist ratio-stage instructions (five gaps or more) behind its producer always
// has one of those seams in between and gets none of its own.
constexpr int kSP128Dist = 24;
// phase B gap (0 .. 31, gap g follows MFMA g): even gaps of entries 0 .. 3 carry an LDS-DMA piece, of entries 8 .. 15 an X load
constexpr bool sp128_b_busy(int gap) { return (gap & 1) == 0 && ((gap >> 1) < 4 || (gap >> 1) >= 8); }
struct SP128PhaseB {
  int first[33];   // moved reciprocals first[g] .. first[g + 1] - 1 sit in gap g
};
constexpr SP128PhaseB sp128_phase_b(int rb) {
  // round-robin from the fourth gap on: phase B's first MFMAs cover the XDL write -> VALU read distance of GEMM1's last, and
  // the first reciprocal (it reads what an asm MFMA wrote) has the seam of entry 1 between itself and that MFMA.
  // The gaps without a load first: one, then a second per odd gap (behind the og = 1 MFMA and the entry's LDS reads:
  // the counted wait follows, so whatever hipcc pads in front of the next MFMA never touches a reciprocal), one, then a second
  // per even gap of entries 4 .. 7; then one and a second per gap that carries a load; a third per odd gap (RB = 64 only)
  int cnt[32] = {};
  int left = rb;
  for (int pass = 0; pass < 7; ++pass)
    for (int g = 3; g < 32; ++g) {
      const int cls = (g & 1) ? 0 : sp128_b_busy(g) ? 2 : 1;
      if (left > 0 && cls == (pass == 6 ? 0 : pass >> 1)) ++cnt[g], --left;
    }
  SP128PhaseB t{};
  for (int g = 0; g < 32; ++g) t.first[g + 1] = t.first[g] + cnt[g];
  return t;
}
struct SP128PhaseA {
  int first[33];   // instructions first[g] .. first[g + 1] - 1 of op[] sit in gap g
  int op[160];     // kind * 64 + index: kind 0 = reciprocal of element x, 1 = multiply of element x, 2 = pack y
};
constexpr SP128PhaseA sp128_phase_a(int rb) {
  SP128PhaseA t{};
  int pos_r[64] = {}, pos_m[64] = {};
  for (int x = 0; x < 64; ++x) pos_r[x] = -1000;   // (the moved ones: long done)
  int nr = rb, nm = 0, nc = 0, pos = 0;
  int cost_left = 2 * (64 - rb) + 64 + 32;
  for (int g = 0; g < 32; ++g) {
    t.first[g] = pos;
    const bool flush = g == 31;
    const int budget = (cost_left + (32 - g) - 1) / (32 - g);
    int used = 0;
    for (int c = 0; c < 2 && nr < 64 && used + 2 <= budget; ++c) {   // at most two reciprocals per gap
      pos_r[nr] = pos;
      t.op[pos++] = nr++;
      used += 2;
    }
    while (nm < 64 && nm < nr && (flush || (used < budget && pos - pos_r[nm] >= kSP128Dist))) {
      pos_m[nm] = pos;
      t.op[pos++] = 64 + nm++;
      ++used;
    }
    while (nc < 32 && 2 * nc + 1 < nm && (flush || (used < budget && pos - pos_m[2 * nc + 1] >= kSP128Dist))) {
      t.op[pos++] = 128 + nc++;
      ++used;
    }
    cost_left -= used;
  }
  t.first[32] = pos;
  return t;
}
template <int RB>
inline constexpr SP128PhaseA kSP128TabA = sp128_phase_a(RB);
template <int RB>
inline constexpr SP128PhaseB kSP128TabB = sp128_phase_b(RB);

template <int OPT, int RB>
__global__ void __launch_bounds__(256, 1) sp128_kernel(const FusedArgs a) {
  using C = SP128Cfg<OPT>;
  static_assert(RB >= 0 && RB <= 64 && RB % 16 == 0, "whole S tiles' worth of units");
  constexpr int R_PAD = C::R_PAD, KS = C::KS, RT = C::RT, ROWB = C::ROWB, IMG = C::IMG, PF = C::PF, N1 = C::N1, N2 = C::N2;
  using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31;   // MFMA column = owner row within a 32-row group
  const int hl = lane >> 5;  // lane half
  const int mb = blockIdx.x / a.nsplit;
  const int ks = blockIdx.x - mb * a.nsplit;
  const int t0 = ks * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.ktiles);
  const int nt = t1 - t0;    // a multiple of 4 (the host rounds tiles_per_split)

  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");  // FP16_OVFL: conversions saturate at 65504
  // clock stamps (nmfmu_step.stamps; layout of nmfmu_sp.h)
  auto stamp = [&](int slot) {
    unsigned long long* dbg = reinterpret_cast<unsigned long long*>(a.debug);
    if (!dbg || wave != 0) return;
    const unsigned long long c = __builtin_amdgcn_s_memtime();
    const unsigned long long r = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
      if (blockIdx.x == 0) {
        dbg[slot * 4 + 0] = c;
        dbg[slot * 4 + 1] = r;
        dbg[slot * 4 + 2] = (unsigned long long)(nt > 0 ? nt : 0);
      }
      dbg[64 + 5 * blockIdx.x + slot] = r;
      if (slot == 2)
        dbg[64 + 5 * blockIdx.x + 4] = ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) |
                                       (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11));
    }
  };
  stamp(2);

  // numerator accumulators of both owner groups: AGPRs for the whole kernel
  f32x16 acc[2][RT];
#pragma unroll
  for (int og = 0; og < 2; ++og)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[og][rt][e] = 0.f;
  static_for<2 * RT>([&](auto rc) {
    f32x16& r = acc[decltype(rc)::value / RT][decltype(rc)::value % RT];
    asm volatile("" : "+a"(r));
  });

  if (nt > 0) {
    const unsigned lds_base =
        __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    const unsigned ldsw = lds_base + (unsigned)wave * (unsigned)(C::NPW * 1024);   // this wave's share of a ring slot: 4 KiB
    const char* xsrc = reinterpret_cast<const char*>(a.xp) + ((size_t)mb * a.ktiles + t0) * (size_t)C::XTILE + (size_t)wave * 8192;
    const char* p1src = reinterpret_cast<const char*>(a.p1_hi) + (size_t)t0 * IMG;
    asm volatile("" : "+s"(xsrc), "+s"(p1src));   // (the kernel arguments have arrived HERE: no wait of hipcc's inside the loop)
    const unsigned lane16 = (unsigned)lane * 16u;
    const unsigned dv = (unsigned)wave * (unsigned)(C::NPW * 1024) + lane16;   // LDS-DMA source offset of this wave's share
    auto clampt = [&](int t) { return t < nt ? t : nt - 1; };   // tail prefetches re-read the last tile (never used)
    auto panel_src = [&](int t) {
      const char* p = p1src + (size_t)clampt(t) * IMG;
      asm volatile("" : "+s"(p));
      return p;
    };
    auto x_src = [&](int t, int og) {   // 13-bit signed instruction offsets end at 4095: one base per owner group
      const char* p = xsrc + (size_t)clampt(t) * (size_t)C::XTILE + (size_t)og * 4096;
      asm volatile("" : "+s"(p));
      return p;
    };

    // ---- owner fragments (B operand of GEMM1): group og, row m0, rank slice 16 kk + 8 hl .. +7 -- AGPRs
    u32x4 q[2][KS];
#pragma unroll
    for (int og = 0; og < 2; ++og) {
      const int m0 = mb * C::BM + (2 * wave + og) * 32 + j;
      const int sw = P1Swz<R_PAD>::of(m0) << 4;
      const char* row = reinterpret_cast<const char*>(a.a1_hi) + (size_t)m0 * ROWB;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) q[og][kk] = ld16(row + ((kk * 32 + hl * 16) ^ sw));
    }

    // ---- per-lane LDS address registers (the algebra of nmfmu_sp2.h)
    //   GEMM1 (tt, kk):        ga[kk] + 16 tt ROWB + slot IMG
    //   GEMM2 (tt, m2, h, rt): gb[2 m2 + h][rt] + (16 tt + 8 m2 + 4 h) ROWB + slot IMG
    const int row0 = 32 * ((j >> 2) & 1) + (j & 3) + 4 * (j >> 3);
    const int sw0 = P1Swz<R_PAD>::of(row0);
    int ga[KS];
#pragma unroll
    for (int v = 0; v < KS; ++v) ga[v] = row0 * ROWB + (((2 * v + hl) ^ sw0) << 4);
    const int grp = lane >> 4, s16 = lane & 15;
    const int cslot = 2 * (grp & 1) + ((s16 & 3) >> 1), lr = (s16 >> 2) & 3;
    int gb[4][RT];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int p = 0; p < RT; ++p)
        gb[c][p] = (32 * (grp >> 1) + (s16 >> 2)) * ROWB + (((cslot ^ c) | ((lr ^ p) << 2)) << 4) + 8 * (s16 & 1);

    f32x16 epsv;   // accumulator seed (eps of nmf.py:65), laundered so that hipcc keeps it resident (see nmfmu_pp.h)
#pragma unroll
    for (int e = 0; e < 16; ++e) epsv[e] = kEps;
    asm volatile("" : "+v"(epsv));

    f32x16 S[2][2][2];        // [buffer][owner group][S^T tile]
    u32x4 xb[2][2][4];        // [X(even tiles) / X(odd tiles)][owner group][chunk]
    uint32_t gn[2][2][8];     // [owner group][S^T tile]: ratios of the tile whose GEMM2 comes next, packed fp16
    u32x4 r128[PF];           // operand ring, GEMM1 entries
    u32x2 rlo[PF], rhi[PF];   // operand ring, GEMM2 entries (two transposing reads each)
    float er[4];              // ratio-stage temporaries

    auto dma_piece = [&](const char* src_tile, auto pc, auto slotc) {
      // the instruction offset moves the LDS destination AND the global source (nmfmu_sp2.h)
      constexpr int p = decltype(pc)::value, off = decltype(slotc)::value * IMG;
      const unsigned vo = dv, lw = ldsw;
      asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%4"
                   :
                   : "v"(vo), "s"(src_tile), "s"(lw), "n"(off), "n"(p * 1024)
                   : "memory", "m0", "scc");
    };
    auto load_x1 = [&](const char* src, u32x4(&x)[4], auto qc) {   // one 16-byte chunk per lane (1 KiB per wave)
      constexpr int qi = decltype(qc)::value;
      const unsigned l16 = lane16;
      u32x4& dst = x[qi];
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 nt" : "=&v"(dst) : "v"(l16), "s"(src), "n"(qi * 1024) : "memory");
    };
    auto wait_x = [&](auto cntc, u32x4(&x)[2][4]) {   // counted wait that makes an X buffer readable
      asm volatile("s_waitcnt vmcnt(%8)"
                   : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[0][2]), "+v"(x[0][3]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[1][2]), "+v"(x[1][3])
                   : "n"(decltype(cntc)::value)
                   : "memory");
    };
    auto barrier = [&]() { asm volatile("s_barrier" ::: "memory"); };
    // ratio-stage instruction k of the tile in S[sb] / xb[sb]: groups of four elements g = (og, tt, d) as in nmfmu_pp.h --
    // 4 x v_rcp_f32, 4 x v_fma_mix_f32 (fp16 half of the X word x fp32 reciprocal), 2 x v_cvt_pk_f16_f32.  No reciprocal
    // is consumed by the instruction right behind it (trans -> VALU forwarding).
    auto ratio_op = [&](auto kc, auto sbc) {
      constexpr int k = decltype(kc)::value, sb = decltype(sbc)::value, GO = C::GOPS;
      constexpr int g = k / GO, pos = k % GO, og = g >> 3, tt = (g >> 2) & 1, d = 2 * (g & 3);
      if constexpr (pos < 4) {
        float& r = er[pos];
        const float sv = S[sb][og][tt][2 * d + pos];
        asm volatile("v_rcp_f32 %0, %1" : "=v"(r) : "v"(sv));
      } else if constexpr (pos < 8) {
        constexpr int p = pos - 4;
        float& r = er[p];
        const uint32_t w = xb[sb][og][2 * tt + (d >> 2)][(d & 3) + (p >> 1)];
        if constexpr ((p & 1) == 0) asm volatile("v_fma_mix_f32 %0, %1, %0, 0 op_sel_hi:[1,0,0]" : "+v"(r) : "v"(w));
        else asm volatile("v_fma_mix_f32 %0, %1, %0, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(w));
      } else {
        constexpr int h = pos - 8;
        uint32_t& g2 = gn[og][tt][d + h];
        const float e0 = er[2 * h], e1 = er[2 * h + 1];
        asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(g2) : "v"(e0), "v"(e1));
      }
    };
    // RB > 0: the same three instructions per element, in place on the S register, addressed by the tables' element x /
    // pack y (unit order above); tile in S[sb] / xb[sb]
    auto rcp_x = [&](auto xc, auto sbc) {
      constexpr int x = decltype(xc)::value, sb = decltype(sbc)::value, u = x >> 2, pos = x & 3;
      constexpr int tt = u >> 3, og = (u >> 2) & 1, d = 2 * (u & 3);
      float r = S[sb][og][tt][2 * d + pos];
      asm volatile("v_rcp_f32 %0, %0" : "+v"(r));
      S[sb][og][tt][2 * d + pos] = r;
    };
    auto mul_x = [&](auto xc, auto sbc) {
      constexpr int x = decltype(xc)::value, sb = decltype(sbc)::value, u = x >> 2, p = x & 3;
      constexpr int tt = u >> 3, og = (u >> 2) & 1, d = 2 * (u & 3);
      float r = S[sb][og][tt][2 * d + p];
      const uint32_t w = xb[sb][og][2 * tt + (d >> 2)][(d & 3) + (p >> 1)];
      if constexpr ((p & 1) == 0) asm volatile("v_fma_mix_f32 %0, %1, %0, 0 op_sel_hi:[1,0,0]" : "+v"(r) : "v"(w));
      else asm volatile("v_fma_mix_f32 %0, %1, %0, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(w));
      S[sb][og][tt][2 * d + p] = r;
    };
    auto pack_y = [&](auto yc, auto sbc) {
      constexpr int y = decltype(yc)::value, sb = decltype(sbc)::value, u = y >> 1, h = y & 1;
      constexpr int tt = u >> 3, og = (u >> 2) & 1, d = 2 * (u & 3);
      uint32_t& g2 = gn[og][tt][d + h];
      const float e0 = S[sb][og][tt][2 * d + 2 * h], e1 = S[sb][og][tt][2 * d + 2 * h + 1];
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(g2) : "v"(e0), "v"(e1));
    };
    auto table_op = [&](auto cc, auto sbc) {   // instruction cc of the phase A table
      constexpr int code = kSP128TabA<RB>.op[decltype(cc)::value], kind = code >> 6;
      using I = std::integral_constant<int, code & 63>;
      if constexpr (kind == 0) rcp_x(I{}, sbc);
      else if constexpr (kind == 1) mul_x(I{}, sbc);
      else pack_y(I{}, sbc);
    };
    // the moved reciprocals of the tile in S[sb], gap `gap` of phase B
    auto rcp_gap = [&](auto gapc, auto sbc) {
      constexpr int gi = decltype(gapc)::value, lo = kSP128TabB<RB>.first[gi], n = kSP128TabB<RB>.first[gi + 1] - lo;
      static_for<n>([&](auto cc) { rcp_x(std::integral_constant<int, lo + decltype(cc)::value>{}, sbc); });
    };
    // the LDS reads of a stream entry into ring slot rs.  G1 entry k: tt = k & 1, kk = k >> 1; G2 entry k: rt = k % RT,
    // (tt, m2) = k / RT.  slotc = panel ring slot of the entry's tile.
    auto issue_g1 = [&](auto kc, auto slotc, auto rsc) {
      constexpr int k = decltype(kc)::value, tt = k & 1, kk = k >> 1, rs = decltype(rsc)::value;
      u32x4& dst = r128[rs];
      const int ad = ga[kk];
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(ad), "n"(tt * 16 * ROWB + decltype(slotc)::value * IMG));
    };
    auto issue_g2 = [&](auto kc, auto slotc, auto rsc) {
      constexpr int k = decltype(kc)::value, rt = k % RT, c4 = k / RT, tt = c4 >> 1, m2 = c4 & 1, rs = decltype(rsc)::value;
      constexpr int o0 = (16 * tt + 8 * m2) * ROWB + decltype(slotc)::value * IMG;
      u32x2 &dlo = rlo[rs], &dhi = rhi[rs];
      const int a0 = gb[2 * m2][rt], a1 = gb[2 * m2 + 1][rt];
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dlo) : "v"(a0), "n"(o0));
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dhi) : "v"(a1), "n"(o0 + 4 * ROWB));
    };
    auto mfma_g1 = [&](auto kc, auto nbc, auto rsc, auto ogc) {   // S[nb][og][tt] (+)= panel fragment x owner fragment (og, kk)
      constexpr int k = decltype(kc)::value, tt = k & 1, kk = k >> 1, nb = decltype(nbc)::value, rs = decltype(rsc)::value;
      constexpr int og = decltype(ogc)::value;
      f32x16& sd = S[nb][og][tt];
      const u32x4 pa = r128[rs], qo = q[og][kk];
      const f32x16 seed = epsv;
      if constexpr (kk == 0) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(sd) : "v"(pa), "a"(qo), "v"(seed));
      else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(sd) : "v"(pa), "a"(qo));
    };
    auto mfma_g2 = [&](auto kc, auto rsc, auto ogc) {             // acc[og][rt] += ratios (og, tt, m2) x transposed panel fragment
      constexpr int k = decltype(kc)::value, rt = k % RT, c4 = k / RT, tt = c4 >> 1, m2 = c4 & 1, rs = decltype(rsc)::value;
      constexpr int og = decltype(ogc)::value;
      const u32x4 nh = {gn[og][tt][4 * m2], gn[og][tt][4 * m2 + 1], gn[og][tt][4 * m2 + 2], gn[og][tt][4 * m2 + 3]};
      const u32x4 bh = {rlo[rs][0], rlo[rs][1], rhi[rs][0], rhi[rs][1]};
      f32x16& ad = acc[og][rt];
      asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(ad) : "v"(nh), "v"(bh));
    };
    auto issue_entry = [&](auto nc, auto lastc) {
      constexpr int n = decltype(nc)::value;
      constexpr SPEnt e = sp_entry<N1, N2>(n, decltype(lastc)::value);
      using RS = std::integral_constant<int, n % PF>;
      if constexpr (e.g1) issue_g1(std::integral_constant<int, e.k>{}, std::integral_constant<int, (e.it + 1) & 3>{}, RS{});
      else issue_g2(std::integral_constant<int, e.k>{}, std::integral_constant<int, e.it & 3>{}, RS{});
    };
    // ratio-stage instructions of MFMA gap `gap` (0 .. 31) of phase A: NEL / 32 each
    auto ratio_gap = [&](auto gapc, auto sbc) {
      constexpr int gi = decltype(gapc)::value, per = C::NEL / 32;
      static_assert(C::NEL % 32 == 0, "whole instructions per gap");
      if constexpr (RB == 0) {
        static_for<per>([&](auto cc) { ratio_op(std::integral_constant<int, gi * per + decltype(cc)::value>{}, sbc); });
      } else {
        constexpr int lo = kSP128TabA<RB>.first[gi], n = kSP128TabA<RB>.first[gi + 1] - lo;
        static_for<n>([&](auto cc) { table_op(std::integral_constant<int, lo + decltype(cc)::value>{}, sbc); });
      }
    };
    // per-phase clock sums (diagnostic builds only: -DNMFMU_SP128_PHASE_STAMPS; tools/sp128_phases.py).  Every boundary reads
    // the shader clock and drains the LDS counter for it, so the build is for the split between the phases, not for timing.
#ifdef NMFMU_SP128_PHASE_STAMPS
    unsigned long long ph_sum[2] = {0, 0}, ph_last = __builtin_amdgcn_s_memtime();
    auto phase_end = [&](int which) {   // the phase that ends here: 0 = A, 1 = B
      const unsigned long long c = __builtin_amdgcn_s_memtime();
      ph_sum[which] += c - ph_last;
      ph_last = c;
    };
    auto phase_reset = [&]() { ph_last = __builtin_amdgcn_s_memtime(); };
#else
    auto phase_end = [&](int) {};
    auto phase_reset = [&]() {};
#endif

    // ---- one group of four tiles i0 .. i0+3 (i0 a multiple of 4: ring slot = it, S / X buffer = it & 1)
    auto group = [&](int i0, auto lastc) {
      constexpr bool last = decltype(lastc)::value;
      constexpr int LEN = sp_group_len<N1, N2>(last);
      const char* dsrc = nullptr;   // panel tile i0+it+3 / X tile i0+it+2: formed at the start of iteration it's phase A,
      const char* xs0 = nullptr;    // read by its phase B (an SGPR base must be older than a few wait states at its VMEM use)
      const char* xs1 = nullptr;
      static_for<PF>([&](auto pc) { issue_entry(pc, lastc); });
      static_for<LEN>([&](auto nc) {
        constexpr int n = decltype(nc)::value;
        constexpr SPEnt e = sp_entry<N1, N2>(n, last);
        constexpr bool final_it = last && e.it == 3;
        using RS = std::integral_constant<int, n % PF>;
        using K = std::integral_constant<int, e.k>;
        using SB = std::integral_constant<int, e.it & 1>;
        using OG0 = std::integral_constant<int, 0>;
        using OG1 = std::integral_constant<int, 1>;
        if constexpr (final_it && e.k == 0)   // last tile: no GEMM1 to hide the ratio stage behind
          static_for<C::NEL - RB>([&](auto kc) {
            if constexpr (RB == 0) ratio_op(kc, SB{});
            else table_op(kc, SB{});
          });
        if constexpr (e.k == 0) phase_end(e.g1 || final_it ? 1 : 0);
        if constexpr (RB > 0 && e.g1 && e.k == 0) {
          // (RB > 0: the scalar upkeep sits at the seam in front of the entry's first MFMA, never between its two MFMAs --
          // hipcc's own instructions and the pads it owes the MFMA chains then fall behind a counted wait, not a ratio op)
          dsrc = panel_src(i0 + e.it + 3);
          xs0 = x_src(i0 + e.it + 2, 0);
          xs1 = x_src(i0 + e.it + 2, 1);
        }
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(sp_younger<N1, N2, PF>(n, last)));
        if constexpr (e.g1) {
          // ---- phase A(it): GEMM1 of tile i0+it+1, ratio stage of tile i0+it
          using NB = std::integral_constant<int, (e.it + 1) & 1>;
          mfma_g1(K{}, NB{}, RS{}, OG0{});
          if constexpr (RB == 0 && e.k == 0) {
            dsrc = panel_src(i0 + e.it + 3);
            xs0 = x_src(i0 + e.it + 2, 0);
            xs1 = x_src(i0 + e.it + 2, 1);
          }
          ratio_gap(std::integral_constant<int, 2 * e.k>{}, SB{});
          mfma_g1(K{}, NB{}, RS{}, OG1{});
          if constexpr (n + PF < LEN) issue_entry(std::integral_constant<int, n + PF>{}, lastc);
          ratio_gap(std::integral_constant<int, 2 * e.k + 1>{}, SB{});
          if constexpr (e.k == N1 - 1) {
            // panel tile i0+it+2 (issued a tile ago) has landed: leaves this wave's 8 youngest loads (X) in flight
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            barrier();
          }
        } else {
          // ---- phase B(it): GEMM2 of tile i0+it; panel tile i0+it+3 into the slot tile i0+it-1 has vacated, X(i0+it+2)
          // into the buffer the ratio stage has just consumed (the panel pieces first: the counted waits rely on the order)
          mfma_g2(K{}, RS{}, OG0{});
          if constexpr (!final_it) {
            if constexpr (e.k < C::NPW) dma_piece(dsrc, K{}, std::integral_constant<int, (e.it + 3) & 3>{});
            if constexpr (e.k >= 8 && e.k < 12) load_x1(xs0, xb[e.it & 1][0], std::integral_constant<int, e.k - 8>{});
            if constexpr (e.k >= 12) load_x1(xs1, xb[e.it & 1][1], std::integral_constant<int, e.k - 12>{});
            // the first RB reciprocals of tile i0+it+1, in place in S[(it + 1) & 1] (phase B(3) serves the next group's tile 0)
            if constexpr (RB > 0) rcp_gap(std::integral_constant<int, 2 * e.k>{}, std::integral_constant<int, (e.it + 1) & 1>{});
          }
          mfma_g2(K{}, RS{}, OG1{});
          if constexpr (n + PF < LEN) issue_entry(std::integral_constant<int, n + PF>{}, lastc);
          if constexpr (RB > 0 && !final_it)
            rcp_gap(std::integral_constant<int, 2 * e.k + 1>{}, std::integral_constant<int, (e.it + 1) & 1>{});
          if constexpr (!final_it && e.k == N2 - 1) {
            // X(i0+it+1) has landed: at most this iteration's 4 panel pieces + 8 X loads stay in flight
            wait_x(std::integral_constant<int, 12>{}, xb[(e.it + 1) & 1]);
          }
        }
      });
    };

    // ---- prologue: panel tiles 0 .. 2, X(0), X(1); everything landed and visible; then GEMM1(0) -> S[0]
    {
      static_for<3>([&](auto tc) {
        const char* src = panel_src(decltype(tc)::value);
        asm volatile("s_nop 4" ::: "memory");
        static_for<C::NPW>([&](auto pc) { dma_piece(src, pc, tc); });
      });
      const char* x00 = x_src(0, 0);
      const char* x01 = x_src(0, 1);
      const char* x10 = x_src(1, 0);
      const char* x11 = x_src(1, 1);
      asm volatile("s_nop 4" ::: "memory");
      static_for<4>([&](auto qc) { load_x1(x00, xb[0][0], qc); });
      static_for<4>([&](auto qc) { load_x1(x01, xb[0][1], qc); });
      static_for<4>([&](auto qc) { load_x1(x10, xb[1][0], qc); });
      static_for<4>([&](auto qc) { load_x1(x11, xb[1][1], qc); });
      wait_x(std::integral_constant<int, 0>{}, xb[0]);
      wait_x(std::integral_constant<int, 0>{}, xb[1]);
      static_for<2 * KS>([&](auto kc) {   // owner fragments -> AGPRs
        u32x4& r = q[decltype(kc)::value / KS][decltype(kc)::value % KS];
        asm volatile("" : "+a"(r));
      });
      barrier();
      using Z = std::integral_constant<int, 0>;
      static_for<PF>([&](auto pc) { issue_g1(pc, Z{}, pc); });
      static_for<N1>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int younger = (N1 - 1 - k) < (PF - 1) ? (N1 - 1 - k) : (PF - 1);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(younger));
        mfma_g1(kc, Z{}, std::integral_constant<int, k % PF>{}, Z{});
        mfma_g1(kc, Z{}, std::integral_constant<int, k % PF>{}, std::integral_constant<int, 1>{});
        if constexpr (k + PF < N1) issue_g1(std::integral_constant<int, k + PF>{}, Z{}, std::integral_constant<int, k % PF>{});
      });
      asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");   // XDL write -> VALU read of S (asm MFMAs are not padded)
      static_for<RB>([&](auto xc) { rcp_x(xc, Z{}); });       // tile 0's share of phase B(-1)
    }
    stamp(0);
    phase_reset();
    int i0 = 0;
    for (; i0 + 4 < nt; i0 += 4) group(i0, std::false_type{});
    group(i0, std::true_type{});
    phase_end(1);
#ifdef NMFMU_SP128_PHASE_STAMPS
    if (a.debug && wave == 0 && blockIdx.x == 0 && lane == 0) {   // [16] phase A cycles (nt - 1 phases), [17] phase B cycles (nt)
      unsigned long long* dbg = reinterpret_cast<unsigned long long*>(a.debug);
      dbg[16] = ph_sum[0], dbg[17] = ph_sum[1], dbg[18] = (unsigned long long)nt;
    }
#endif
    stamp(1);
    // XDL write -> VALU read of the accumulators; the clamped tail prefetches: nothing may land in LDS / registers after this
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    wait_x(std::integral_constant<int, 0>{}, xb[0]);
    wait_x(std::integral_constant<int, 0>{}, xb[1]);
  }
  __syncthreads();               // LDS is reused by the epilogue

  // ---------------- epilogue: the ping-pong kernel's (nmfmu_pp.h), every wave in the role of its waves 2 w (og = 0) and
  // 2 w + 1 (og = 1): same staging tiles, same chunk order per lane, same order of the column-sum partials.
  int tid_e = tid;
  asm volatile("" : "+v"(tid_e));
  const int lane_e = tid_e & 63, j_e = lane_e & 31, hl_e = lane_e >> 5;
  // accumulator register e of lane (j_e, hl_e): row (e & 3) + 8 (e >> 2) + 4 hl_e of the group, column 32 rt + j_e
  if (a.fuse_apply) {
    constexpr int LDT = R_PAD;
    constexpr int SP = R_PAD / 8;            // sixteen-byte image slots (8 ranks) per row
    constexpr int NCH = (32 * SP) / 64;      // (row, slot) chunks per lane and group
    const int slot_e = lane_e % SP, rl0 = lane_e / SP;
    float den8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) den8[k] = a.kl_den[slot_e * 8 + k];
    const bool vec = (a.rank & 3) == 0;
    bool clamped = false;   // fp16 images saturate at 65504 (MODE.FP16_OVFL): reported through a.status
    static_for<2 * RT>([&](auto rc) {
      constexpr int og = decltype(rc)::value / RT, rt = decltype(rc)::value % RT;
      float* tile = reinterpret_cast<float*>(smem) + (2 * wave + og) * (32 * LDT);
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[((e & 3) + 8 * (e >> 2) + 4 * hl_e) * LDT + rt * 32 + j_e] = acc[og][rt][e];
    });
    __syncthreads();
    const bool plain = a.l1 <= 0.f && a.l2 <= 0.f && a.gamma == 1.f && a.rank == R_PAD && mb * C::BM + C::BM <= a.M;
    float csum8[2][8], rden8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) rden8[k] = 1.f / den8[k];   // (the branch-free form's multipliers; unused by the general form)
#pragma unroll
    for (int og = 0; og < 2; ++og) {
      float* tile = reinterpret_cast<float*>(smem) + (2 * wave + og) * (32 * LDT);
      const int mrow0 = mb * C::BM + (2 * wave + og) * 32;
#pragma unroll
      for (int k = 0; k < 8; ++k) csum8[og][k] = 0.f;
      if (plain) {
#pragma unroll 4
        for (int i = 0; i < NCH; ++i) {
          const int rl = i * (64 / SP) + rl0, row = mrow0 + rl, r0 = slot_e * 8;
          float* trow = tile + rl * LDT + r0;
          float* frow = a.f + (size_t)row * R_PAD + r0;
          float fv[8], nm[8];
          *reinterpret_cast<float4*>(fv) = *reinterpret_cast<const float4*>(frow);
          *reinterpret_cast<float4*>(fv + 4) = *reinterpret_cast<const float4*>(frow + 4);
          *reinterpret_cast<float4*>(nm) = *reinterpret_cast<const float4*>(trow);
          *reinterpret_cast<float4*>(nm + 4) = *reinterpret_cast<const float4*>(trow + 4);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            // the column sum takes the product unrounded (one fused multiply-add), as hipcc contracts it in the ping-pong
            // kernel's epilogue: written out so that the two kernels cannot drift apart by a compiler's choice
            const float mult = (fmaxf(nm[k], 0.f) + kEps) * rden8[k];
            csum8[og][k] = __builtin_fmaf(fv[k], mult, csum8[og][k]);
            fv[k] *= mult;
            clamped |= fv[k] > 65504.f;
          }
          *reinterpret_cast<float4*>(frow) = *reinterpret_cast<const float4*>(fv);
          *reinterpret_cast<float4*>(frow + 4) = *reinterpret_cast<const float4*>(fv + 4);
          if (a.o2_hi) {   // (the updated tile feeds the transposed image only)
            *reinterpret_cast<float4*>(trow) = *reinterpret_cast<const float4*>(fv);
            *reinterpret_cast<float4*>(trow + 4) = *reinterpret_cast<const float4*>(fv + 4);
          }
          u32x4 hi;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) hi[qq] = pack_op<OPT>(fv[2 * qq], fv[2 * qq + 1]);
          *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.o1_hi) + p1_offset(row, r0, R_PAD)) = hi;
        }
      } else {
#pragma unroll 2
        for (int i = 0; i < NCH; ++i) {
          const int rl = i * (64 / SP) + rl0, row = mrow0 + rl, r0 = slot_e * 8;
          float* trow = tile + rl * LDT + r0;
          float* frow = a.f + (size_t)row * a.rank + r0;
          float fv[8], nm[8];
          *reinterpret_cast<float4*>(nm) = *reinterpret_cast<const float4*>(trow);
          *reinterpret_cast<float4*>(nm + 4) = *reinterpret_cast<const float4*>(trow + 4);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool in = row < a.M && r0 + 4 * h < a.rank;
            if (in && vec) {
              *reinterpret_cast<float4*>(fv + 4 * h) = *reinterpret_cast<const float4*>(frow + 4 * h);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k) fv[4 * h + k] = (in && r0 + 4 * h + k < a.rank) ? frow[4 * h + k] : 0.f;
            }
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float neg = fmaxf(nm[k], 0.f) + kEps;
            float pos = den8[k];
            if (a.l1 > 0.f) pos += a.l1;
            if (a.l2 > 0.f) pos += a.l2 * fv[k];
            float mult = neg / pos;
            if (a.gamma != 1.f) mult = mu_pow(mult, a.gamma);
            // padding rows / ranks stay exactly 0 (their denominators may be 0: 0 * inf)
            fv[k] = (row < a.M && r0 + k < a.rank) ? fv[k] * mult : 0.f;
            csum8[og][k] += fv[k];
            clamped |= fv[k] > 65504.f;
          }
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool in = row < a.M && r0 + 4 * h < a.rank;
            if (in && vec) {
              *reinterpret_cast<float4*>(frow + 4 * h) = *reinterpret_cast<const float4*>(fv + 4 * h);
            } else if (in) {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (r0 + 4 * h + k < a.rank) frow[4 * h + k] = fv[4 * h + k];
            }
          }
          *reinterpret_cast<float4*>(trow) = *reinterpret_cast<const float4*>(fv);
          *reinterpret_cast<float4*>(trow + 4) = *reinterpret_cast<const float4*>(fv + 4);
          u32x4 hi;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) hi[qq] = pack_op<OPT>(fv[2 * qq], fv[2 * qq + 1]);
          *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.o1_hi) + p1_offset(row, r0, R_PAD)) = hi;
        }
      }
    }
    if (a.status && __any(clamped) && lane_e == 0) atomicOr(a.status, 1u);
    // transposed image from the updated tiles: 8 consecutive owner rows of one rank = one sixteen-byte slot
    // (a.o2_hi == nullptr: nobody reads the owner's transposed image; the pass and its barrier go)
    if (a.o2_hi) {
      __syncthreads();
#pragma unroll
      for (int og = 0; og < 2; ++og) {
        const float* tile = reinterpret_cast<const float*>(smem) + (2 * wave + og) * (32 * LDT);
        const int mrow0 = mb * C::BM + (2 * wave + og) * 32;
#pragma unroll
        for (int ii = 0; ii < R_PAD / 64; ++ii) {
          const int r = ii * 64 + lane_e;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float* src = tile + (g * 8) * LDT + r;
            u32x4 hi;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) hi[qq] = pack_op<OPT>(src[(2 * qq) * LDT], src[(2 * qq + 1) * LDT]);
            *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.o2_hi) + p2_offset(mrow0 + g * 8, r, R_PAD)) = hi;
          }
        }
      }
    }
    __syncthreads();
    // partial column sums of this workgroup's rows: the lanes sharing a slot, then the eight groups (the ping-pong kernel's order)
    float* red = reinterpret_cast<float*>(smem);  // [8][R_PAD]
#pragma unroll
    for (int og = 0; og < 2; ++og)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float tot = csum8[og][k];
        tot += __shfl_xor(tot, 32, 64);
        tot += __shfl_xor(tot, 16, 64);
        if (lane_e < SP) red[(2 * wave + og) * R_PAD + slot_e * 8 + k] = tot;
      }
    __syncthreads();
    for (int r = tid_e; r < R_PAD; r += C::THREADS) {
      float tot = (red[r] + red[R_PAD + r]) + (red[2 * R_PAD + r] + red[3 * R_PAD + r]);
      tot += (red[4 * R_PAD + r] + red[5 * R_PAD + r]) + (red[6 * R_PAD + r] + red[7 * R_PAD + r]);
      a.colsum_part[(size_t)mb * R_PAD + r] = tot;
    }
  } else {
    static_for<2 * RT>([&](auto rc) {
      constexpr int og = decltype(rc)::value / RT, rt = decltype(rc)::value % RT;
      const size_t slab = ((size_t)ks * a.M_pad + (size_t)(mb * C::BM + (2 * wave + og) * 32)) * R_PAD;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * hl_e;
        a.slab_num[slab + (size_t)row * R_PAD + rt * 32 + j_e] = acc[og][rt][e];
      }
    });
  }
  if (a.debug) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the epilogue's stores have left the CU
  stamp(3);
}

template <int OPT, int RB>
int launch_sp128_one(const FusedArgs& a, int grid, hipStream_t s) {
  using C = SP128Cfg<OPT>;
  return launch_with_dynamic_lds<sp128_kernel<OPT, RB>, C::THREADS, C::LDS_BYTES>(dim3(grid), s, a);
}

// Host-side launcher (nmfmu_inst_sp128.hip).  Serves beta == 1, fp16 operands and target, padded rank 128, 256-row tiles.
int launch_sp128(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s);
// ... the RB = 0 schedule, kept as the A/B arm of NMFMU_STAGE_DMA_SP128_RB0 (nmfmu_inst_sp128_rb0.hip)
int launch_sp128_rb0(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s);
bool sp128_available(int r_pad, int opt, int mode);

}  // namespace nmfmu
