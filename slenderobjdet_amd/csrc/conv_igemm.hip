// Implicit-GEMM convolution on MFMA for gfx950 (CDNA4): forward, data-gradient and weight-gradient.
//
// Replaces the ATen/cuDNN convolutions the reference reaches through detectron2's ResNet/FPN and through
// FCOSHead (reference: slender_det/modeling/meta_arch/fcos/fcosv2.py:277-381, backbone/fpn.py:94-115).
//
// Layout: activations NHWC bf16, weights [Cout][R][S][Cin] bf16 ("KRSC"; for dgrad the host supplies the
// transposed copy [Cin][R][S][Cout]).  GEMM view: rows of the MFMA "A" operand are output channels (q),
// columns of the "B" operand are pixels (p), the contraction index is (tap, channel), 64 per K-step.
// Both operands are contraction-contiguous in memory, so tiles are staged HBM->LDS with
// buffer_load_dwordx4 ... lds (no VGPR round trip); padding/out-of-range lanes use an out-of-bounds
// buffer offset and the hardware returns zeros.  LDS rows are 128 B; the 16-B chunk index is XOR-swizzled
// on the SOURCE side ((row>>1)&7) so that ds_read_b128 fragment reads are bank-conflict free.
//
// wgrad contracts over pixels, which is the slow axis of both operands: tiles are staged [pixel][128 ch]
// and fragments are fetched with ds_read_b64_tr_b16 (hardware transpose), swizzled at 32-B granularity.
//
// Kernels and their plain launchers only: which shapes come here (and with which tile) is decided in conv_dispatch.hip.
#include "conv_args.h"
#include <type_traits>

using namespace sodconv;

namespace {

template <int MODE, bool GENERIC, int WQ, int WP, int FQ, int FP, bool OUT_F32, int BK, int NSTAGE>
__global__ __launch_bounds__(64 * WQ * WP, (WQ * WP == 4 && BK == 32 && NSTAGE == 2) ? 4 : 2) void conv_igemm_kernel(const ConvArgs a) {
  constexpr int NW = WQ * WP;                  // waves per workgroup (4 or 8)
  constexpr int BQ = WQ * FQ * 16, BP = WP * FP * 16;
  constexpr int ROWB = BK * 2;                 // bytes per LDS row (one pixel / one output channel, BK contraction elements)
  constexpr int CPR = BK / 8;                  // 16-B chunks per row (8 or 4)
  constexpr int RPI = 64 / CPR;                // rows one wave instruction (1 KiB) covers
  constexpr int RPP = NW * RPI;                // rows per pass of all waves
  constexpr int SWS = (BK == 64) ? 1 : 2;      // swizzle = (row >> SWS) & (CPR-1)
  constexpr int W_TILE = BQ * ROWB, X_TILE = BP * ROWB, STAGE = W_TILE + X_TILE;
  constexpr int XI = BP / RPP;   // X rows per thread
  static_assert(BK == 64 || BK == 32, "BK");
  static_assert(BP % RPP == 0, "tile rows");
  constexpr bool WFULL = (BQ % RPP == 0);     // every wave stages weight rows in every pass: no wave-dependent branch in the K loop
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  static_assert(NSTAGE >= 2 && NSTAGE <= 6, "LDS ring depth");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  if (a.flags & F_REVERSE) bid = gridDim.x - 1 - bid;
  const int qt = bid % a.nq_tiles;
  int pt = bid / a.nq_tiles;   // q fastest: neighbours share the X tile
  int lv = 0;
#pragma unroll
  for (int i = 1; i < MAXLEV; ++i)
    if (i < a.nlev && pt >= a.lev[i].tile0) lv = i;
  const LevelGeo& g = a.lev[lv];
  pt -= g.tile0;
  const int q0 = qt * BQ, p0 = g.pstart + pt * BP;
  const int gP = g.P, gHs = g.Hs, gWs = g.Ws;
  const uint32_t Cp = (uint32_t)a.Cpitch;               // source channels per pixel (= Cred unless a channel window is on)
  const uint32_t cw0 = a.cwin ? (uint32_t)q0 : 0u;      // window mode: this q-tile contracts over the source channels at its own offset
  const bool pitched = a.Cpitch < a.Cred;               // wave-uniform: only sod_conv2d_dgrad_ml_kpitch launches

  auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, a.w_bytes, 0x00020000);
  auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.src), 0, g.src_bytes, 0x00020000);

  // ---- per-thread staging geometry (rows are fixed for the whole K loop) ----
  const int srow = lane / CPR;                                  // row inside one wave instruction
  const int spos = lane % CPR;                                  // 16-B slot inside the row
  // tile_row = (i*4 + wave)*RPI + srow ; swizzle = (tile_row >> SWS) & (CPR-1)
  const int sswz = (BK == 64) ? ((lane >> 4) | ((wave & 1) << 2)) : ((srow >> 2) & 3);
  const int schunk = spos ^ sswz;                               // logical chunk this lane fetches
  int xh[XI], xw[XI];
  uint32_t xoff[XI];
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int row = (i * NW + wave) * RPI + srow;
    const uint32_t p = p0 + row;
    if (p < (uint32_t)gP) {
      const uint32_t n = fd_div(p, g.div_hw);
      const uint32_t rem = p - n * g.div_hw.d;
      const uint32_t ph = fd_div(rem, g.div_w);
      const uint32_t pw = rem - ph * g.div_w.d;
      if (MODE == MODE_FWD) { xh[i] = (int)ph * a.stride - a.pad; xw[i] = (int)pw * a.stride - a.pad; }
      else                  { xh[i] = (int)ph + a.pad;            xw[i] = (int)pw + a.pad; }
      xoff[i] = n * (uint32_t)g.src_img_stride;
    } else {
      xh[i] = -(1 << 28); xw[i] = -(1 << 28); xoff[i] = 0;
    }
  }

  // branch-free source coordinate: returns all-ones mask when valid
  auto src_coord = [&](int base, int tapo, int lim, int& out) -> uint32_t {
    if (MODE == MODE_FWD) {
      out = base + tapo * a.dil;
      return (uint32_t) - (int)((unsigned)out < (unsigned)lim);
    } else {
      const int t = base - tapo * a.dil;
      if (a.stride == 1) {   // wave-uniform
        out = t;
        return (uint32_t) - (int)((unsigned)t < (unsigned)lim);
      }
      const uint32_t tt = (uint32_t)(t < 0 ? 0 : t);
      const uint32_t o = fd_div(tt, a.div_stride);
      out = (int)o;
      return (uint32_t) - (int)((t >= 0) & (o * (uint32_t)a.stride == tt) & (o < (uint32_t)lim));
    }
  };

  // LINEAR fast path (the issue port, not the matrix pipe, was the limiter: ~90 VALU per K-step against 32 MFMAs).
  // When the tap is uniform per K-step (!GENERIC) and the source coordinate is affine in the tap (fwd, or dgrad with
  // stride 1), the byte offset of a row is rowbase + tapoff(t) with a SCALAR tapoff, and the padding test is one bit of a
  // per-row tap-validity mask computed once here.  Per K-step and row: one add, one shift/and, one select.
  // forward non-generic kernels are always linear (the host routes R*S > 64 to the generic kernel): a compile-time constant there,
  // so the gather path and its branch drop out of the forward K loop
  const bool linear = !GENERIC && (MODE == MODE_FWD || (a.stride == 1 && a.R * a.S <= 64));
  uint32_t rowbase[XI];
  unsigned long long tapmask[XI];
  uint32_t wbase[(BQ + RPP - 1) / RPP];
  if (linear) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      rowbase[i] = (xoff[i] + ((uint32_t)xh[i] * (uint32_t)gWs + (uint32_t)xw[i]) * Cp + cw0 + (uint32_t)schunk * 8u) * 2u;
      // a tap is valid iff its row and its column are: R + S tests and an outer product of the two bit rows instead of R * S tests
      unsigned long long m = 0, colbits = 0;
      for (int s2 = 0; s2 < a.S; ++s2) {
        int w;
        colbits |= (unsigned long long)(src_coord(xw[i], s2, gWs, w) & 1u) << s2;
      }
      for (int r = 0; r < a.R; ++r) {
        int h;
        if (src_coord(xh[i], r, gHs, h) & 1u) m |= colbits << (r * a.S);
      }
      tapmask[i] = m;
    }
#pragma unroll
    for (int j = 0; j < (BQ + RPP - 1) / RPP; ++j) {
      const int row = j * RPP + wave * RPI + srow;
      const int q = q0 + row;
      wbase[j] = (q < a.Nout && row < BQ) ? ((uint32_t)q * (uint32_t)a.Kred + (uint32_t)schunk * 8u) * 2u : SOD_OOB;
    }
  }
  const int tap_sign = (MODE == MODE_FWD) ? 1 : -1;

  auto stage = [&](int t, char* buf) {
#if defined(SOD_IGEMM_ABL) && (SOD_IGEMM_ABL & 2)      // measurement build: no K-loop loads (tools/bench_1x1.py)
    return;
#endif
    if (linear) {
      // both K orders computed with scalar multiply-highs and selected (no branch in the K loop)
      const uint32_t cc = (__umulhi((uint32_t)t, a.div_rs.mul) + (uint32_t)t) >> a.div_rs.shr;
      const uint32_t tap_o = (__umulhi((uint32_t)t, a.div_cpt.mul) + (uint32_t)t) >> a.div_cpt.shr;
      const uint32_t tap = a.tap_inner ? (uint32_t)t - cc * a.div_rs.d : tap_o;
      const int c0 = (a.tap_inner ? (int)cc : t - (int)(tap_o * a.div_cpt.d)) * BK;
      const int r = (int)fd_div(tap, a.div_s);
      const int s2 = (int)tap - r * a.S;
      const uint32_t tapoff = (uint32_t)((tap_sign * (r * a.dil * gWs + s2 * a.dil) * (int)Cp + c0) * 2);   // scalar
      const uint32_t woff = (uint32_t)(((int)tap * a.Cred + c0) * 2);
#pragma unroll
      for (int j = 0; j < (BQ + RPP - 1) / RPP; ++j) {
        if (WFULL || j * RPP + wave * RPI < BQ) {
          const uint32_t voff = (wbase[j] == SOD_OOB) ? SOD_OOB : wbase[j] + woff;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, SOD_LDS(buf + (j * RPP + wave * RPI) * ROWB), 16, voff, 0, 0, 0);
        }
      }
      // a source pitch BELOW the contraction width (sod_conv2d_dgrad_ml_kpitch): chunks past the pixel's last channel are zero fill, never
      // the next pixel's data (whatever follows the buffer may hold NaN bit patterns, and NaN x 0 is NaN)
      const bool cin = !pitched || (c0 + schunk * 8 < (int)Cp);
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        const bool ok = ((tapmask[i] >> tap) & 1ull) && cin;
        const uint32_t voff = ok ? rowbase[i] + tapoff : SOD_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, SOD_LDS(buf + W_TILE + (i * NW + wave) * 1024), 16, voff, 0, 0, 0);
      }
      return;
    }
    // weights: row-major [q][Kred]; K-step t covers flattened contraction [t*BK, (t+1)*BK)
#pragma unroll
    for (int rb = 0; rb < BQ; rb += RPP) {
      if (WFULL || rb + wave * RPI < BQ) {
        const int row = rb + wave * RPI + srow;
        const int q = q0 + row;
        const int kk = t * BK + schunk * 8;
        const uint32_t m = (uint32_t) - (int)((q < a.Nout) & (kk < a.Kred) & (row < BQ));
        const uint32_t off = ((uint32_t)q * (uint32_t)a.Kred + (uint32_t)kk) * 2u;
        const uint32_t voff = (off & m) | (SOD_OOB & ~m);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, SOD_LDS(buf + (rb + wave * RPI) * ROWB), 16, voff, 0, 0, 0);
      }
    }
    int r_u = 0, s_u = 0, c0_u = 0;
    if (!GENERIC) {
      const uint32_t tap = fd_div((uint32_t)t, a.div_cpt);
      c0_u = (t - (int)(tap * a.div_cpt.d)) * BK;
      r_u = (int)fd_div(tap, a.div_s);
      s_u = (int)tap - r_u * a.S;
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      int r, s, c;
      uint32_t m = 0xFFFFFFFFu;
      if (GENERIC) {
        const uint32_t gi = (uint32_t)t * (uint32_t)CPR + (uint32_t)schunk;     // 8-channel chunk index
        const uint32_t tap = fd_div(gi, a.div_cpt);
        c = (int)(gi - tap * a.div_cpt.d) << 3;
        r = (int)fd_div(tap, a.div_s);
        s = (int)tap - r * a.S;
        m = (uint32_t) - (int)(r < a.R);
      } else {
        r = r_u; s = s_u; c = c0_u + schunk * 8;
      }
      int h, w;
      m &= src_coord(xh[i], r, gHs, h);
      m &= src_coord(xw[i], s, gWs, w);
      const uint32_t off = (xoff[i] + ((uint32_t)h * (uint32_t)gWs + (uint32_t)w) * Cp + cw0 + (uint32_t)c) * 2u;
      const uint32_t voff = (off & m) | (SOD_OOB & ~m);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, SOD_LDS(buf + W_TILE + (i * NW + wave) * 1024), 16, voff, 0, 0, 0);
    }
  };

  // ---- fragment read offsets ----
  const int wq = wave / WP, wp = wave % WP;
  const int fr = lane & 15, fg = lane >> 4;
  uint32_t aoff[FQ], boff[FP];
#pragma unroll
  for (int i = 0; i < FQ; ++i) {
    const int row = (wq * FQ + i) * 16 + fr;
    aoff[i] = row * ROWB + ((fg ^ ((row >> SWS) & (CPR - 1))) << 4);
  }
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    const int row = (wp * FP + j) * 16 + fr;
    boff[j] = W_TILE + row * ROWB + ((fg ^ ((row >> SWS) & (CPR - 1))) << 4);
  }

  f32x4_t acc[FQ][FP];
#pragma unroll
  for (int i = 0; i < FQ; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const char* cur) {
#if defined(SOD_IGEMM_ABL) && (SOD_IGEMM_ABL & 1)      // measurement build: no fragment reads, no MFMAs
    acc[0][0][0] += (float)(uintptr_t)cur;
    return;
#endif
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8_t af[FQ], bf[FP];
#pragma unroll
      for (int i = 0; i < FQ; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(cur + (aoff[i] ^ (ks << 6)));
#pragma unroll
      for (int j = 0; j < FP; ++j) bf[j] = *reinterpret_cast<const bf16x8_t*>(cur + (boff[j] ^ (ks << 6)));
#pragma unroll
      for (int i = 0; i < FQ; ++i)
#pragma unroll
        for (int j = 0; j < FP; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  if constexpr (NSTAGE == 2) {
    stage(0, smem);
    for (int t = 0; t < a.T; ++t) {
      __syncthreads();   // drains this wave's LDS-DMA (vmcnt(0)) and orders all waves' reads of the other buffer
      if (t + 1 < a.T) stage(t + 1, smem + ((t + 1) & 1) * STAGE);
      compute(smem + (t & 1) * STAGE);
    }
  } else {
    // NSTAGE-deep LDS ring: the tiles for steps t+1 .. t+NSTAGE-1 are in flight while step t is computed, so a load has NSTAGE-1 full
    // steps to land instead of one (a 32-deep K-step is 256 cycles of MFMA per wave against ~2 k cycles of memory latency: with one
    // step of prefetch every K-step of a short-K 1x1 convolution waited for its operands).  Counted vmcnt keeps the younger stages in
    // flight across the (raw) barrier; every thread issues exactly LPS LDS-DMA loads per stage.
    constexpr int LPS = BQ / RPP + XI;
    constexpr int AHEAD = NSTAGE - 1;
    static_assert(WFULL, "counted vmcnt needs a fixed number of loads per stage");
    static_assert((AHEAD - 1) * LPS <= 63, "vmcnt range");
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
      if (s < a.T) stage(s, smem + s * STAGE);
    int slot = 0;
    for (int t = 0; t < a.T; ++t) {
      int younger = a.T - 1 - t;                 // stages requested after tile t: they may stay in flight
      if (younger > AHEAD - 1) younger = AHEAD - 1;
      switch (younger) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPS) : "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPS) : "memory"); break;
      }
      __builtin_amdgcn_s_barrier();   // tile t has landed for every wave; every wave has finished computing tile t-1
      int nslot = slot + AHEAD; if (nslot >= NSTAGE) nslot -= NSTAGE;
      if (t + AHEAD < a.T) stage(t + AHEAD, smem + nslot * STAGE);   // overwrites the buffer of tile t-1
      compute(smem + slot * STAGE);
      slot = (slot == NSTAGE - 1) ? 0 : slot + 1;
    }
  }

  // ---- epilogue ----
  // The accumulator tile is D[row=q][col=p]: a lane holds 4 consecutive q of ONE pixel, i.e. 8-B pieces scattered over
  // 16 pixel rows.  Stage the wave's tile through LDS (fp32, [pixel][q]) and read it back so that each lane owns 16
  // contiguous output bytes and 4-16 lanes cover one pixel's channel run: residual / mask loads and the stores become
  // full 64-256 B segments.
  const int Nout = a.Nout;
  if ((Nout & 7) == 0) {
    constexpr int QW = FQ * 16;                  // channels per wave tile
    constexpr int EROWB = QW * 4 + 16;           // fp32 row + 16 B pad (keeps 16-B alignment, spreads banks)
    constexpr int NH = 2, FH = FP / NH;          // two halves of FH fragments (FH*16 pixel rows) bound the LDS use
    constexpr int EPL = OUT_F32 ? 4 : 8;         // output elements per lane (16 B)
    constexpr int LPR = QW / EPL;                // lanes per pixel row
    constexpr int ERPP = 64 / LPR;               // pixel rows per pass
    static_assert(FP % NH == 0, "halves");
    __syncthreads();                             // every wave has finished reading the K-loop buffers
    char* wl = smem + wave * (FH * 16 * EROWB);
    const int erow = lane / LPR, eq = (lane % LPR) * EPL;
    const int q = q0 + wq * QW + eq;
    constexpr int NP = FH * 16 / ERPP;           // passes per half
    using RV = typename std::conditional<EPL == 8, bf16x8_t, bf16x4_t>::type;
    const bool qok = q < Nout;
    // bias depends only on the lane's channels: one load for the whole tile
    float bv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) bv[e] = 0.f;
    if ((a.flags & F_BIAS) && qok) {
#pragma unroll
      for (int e = 0; e < EPL; e += 4) {
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(a.bias + q + e);
        bv[e] = b[0]; bv[e + 1] = b[1]; bv[e + 2] = b[2]; bv[e + 3] = b[3];
      }
    }
    GnAcc ga{0.f, 0.f, -1};
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      // Residual / mask operands of ALL passes of this half are requested before the accumulators go through LDS: one exposed
      // memory latency per half instead of two dependent round trips per pass (load -> wait -> store, eight times per tile) -
      // the memory-bound 1x1 expansions of the bottleneck blocks spent most of a block's life there.
      RV resv[NP], maskv[NP];
      size_t drow[NP];
      bool ok[NP];
      int nimg[NP];
      uint32_t mbits[NP];
      bool odd[NP];
      // (image, pixel-in-image) of this lane's first row by one division, the rows of the following passes (ERPP pixels further each) by carry
      const uint32_t pfirst = p0 + (wp * FP + h * FH) * 16 + erow;
      const uint32_t pc0 = pfirst < (uint32_t)gP ? pfirst : 0u;
      uint32_t n_run = fd_div(pc0, g.div_hw);
      uint32_t rem_run = pc0 - n_run * g.div_hw.d;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const uint32_t p = pfirst + (uint32_t)(k * ERPP);
        ok[k] = (p < (uint32_t)gP) && qok;
        drow[k] = 0;
        const uint32_t n = n_run, rem = rem_run;
        rem_run += (uint32_t)ERPP;
        while (rem_run >= g.div_hw.d) { rem_run -= g.div_hw.d; ++n_run; }      // (levels of a few pixels: more than one wrap)
        if (ok[k]) {
          nimg[k] = (int)n;
          drow[k] = (size_t)n * g.dst_img_stride + (size_t)rem * Nout;
          if (a.flags & (F_RES | F_RES_UP2)) {
            size_t res_row;
            if (a.flags & F_RES_UP2) {
              const uint32_t ph = fd_div(rem, g.div_w);
              const uint32_t pw = rem - ph * g.div_w.d;
              res_row = (size_t)n * g.res_img_stride + (size_t)((ph >> 1) * (g.Wp >> 1) + (pw >> 1)) * Nout;
              if constexpr (MODE == MODE_DGRAD && !OUT_F32) odd[k] = (a.flags & F_RES_EVEN) && ((ph | pw) & 1u);   // loaded anyway (no lane-
            } else {                                                                                                // dependent branch), not added
              res_row = (size_t)n * g.res_img_stride + (size_t)rem * Nout;
              if constexpr (MODE == MODE_DGRAD && !OUT_F32) odd[k] = false;
            }
            resv[k] = *reinterpret_cast<const RV*>((const __bf16*)g.res + res_row + q);
          }
          if constexpr (MODE == MODE_DGRAD) {      // forward launches never carry a mask: no registers for it there
            if (a.flags & F_MASK) maskv[k] = *reinterpret_cast<const RV*>((const __bf16*)g.mask + drow[k] + q);
          }
          if constexpr (MODE == MODE_DGRAD && !OUT_F32) {
            if (a.flags & F_MASKBITS) mbits[k] = ((const uint8_t*)g.mask)[(drow[k] + q) >> 3];
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < FH; ++jj)
#pragma unroll
        for (int i = 0; i < FQ; ++i)
          *reinterpret_cast<f32x4_t*>(wl + (jj * 16 + fr) * EROWB + (i * 16 + fg * 4) * 4) = acc[i][h * FH + jj];
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int row = k * ERPP + erow;
        if (ok[k]) {
          float v[EPL];
#pragma unroll
          for (int e = 0; e < EPL; e += 4) {
            const f32x4_t t4 = *reinterpret_cast<const f32x4_t*>(wl + row * EROWB + (eq + e) * 4);
            v[e] = t4[0]; v[e + 1] = t4[1]; v[e + 2] = t4[2]; v[e + 3] = t4[3];
          }
          if (a.flags & F_BIAS) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) v[e] += bv[e];
          }
          if (a.flags & (F_RES | F_RES_UP2)) {
            if constexpr (MODE == MODE_DGRAD && !OUT_F32) {
#pragma unroll
              for (int e = 0; e < EPL; ++e) v[e] += odd[k] ? 0.f : (float)resv[k][e];
            } else {
#pragma unroll
              for (int e = 0; e < EPL; ++e) v[e] += (float)resv[k][e];
            }
          }
          if (a.flags & F_RELU) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) v[e] = fmaxf(v[e], 0.f);
          }
          if constexpr (MODE == MODE_DGRAD) {
            if (a.flags & F_MASK) {
#pragma unroll
              for (int e = 0; e < EPL; ++e) v[e] = ((float)maskv[k][e] > 0.f) ? v[e] : 0.f;
            }
          }
          if constexpr (MODE == MODE_DGRAD && !OUT_F32) {
            if (a.flags & F_MASKBITS) {
#pragma unroll
              for (int e = 0; e < EPL; ++e) v[e] = ((mbits[k] >> e) & 1u) ? v[e] : 0.f;
            }
          }
#if defined(SOD_IGEMM_ABL) && (SOD_IGEMM_ABL & 8)      // measurement build: no output stores (unless a value no input produces shows up)
          if (v[0] != 12345.678f) continue;
#endif
          if constexpr (OUT_F32) {
            sod_store16((float*)g.dst + drow[k] + q, f32x4_t{v[0], v[1], v[2], v[3]});
          } else {
            bf16x8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
            sod_store16((__bf16*)g.dst + drow[k] + q, o);
            if constexpr (MODE == MODE_FWD) {
              if (a.flags & F_WBITS) {
                uint32_t b = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) b |= ((float)o[e] > 0.f ? 1u : 0u) << e;
                ((uint8_t*)g.bits)[(drow[k] + q) >> 3] = (uint8_t)b;
              }
            }
            if constexpr (MODE == MODE_FWD) { if (a.flags & F_GNSTATS) gn_acc_add(ga, nimg[k], o, g.gn_sum, a.gn_G, q >> 3); }
          }
        }
      }
    }
    if constexpr (!OUT_F32 && MODE == MODE_FWD) {
      if (a.flags & F_GNSTATS)
        gn_acc_finish<LPR>(ga, p0 + wp * FP * 16, p0 + wp * FP * 16 + FP * 16 - 1, (uint32_t)gP, g.div_hw, g.gn_sum, a.gn_G, q >> 3, qok, lane);
    }
    return;
  }

  // scalar fallback (Nout not a multiple of 8): lane holds 4 consecutive q for one pixel
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    const uint32_t p = p0 + (wp * FP + j) * 16 + fr;
    if (p >= (uint32_t)gP) continue;
    const uint32_t n = fd_div(p, g.div_hw);
    const uint32_t rem = p - n * g.div_hw.d;
    size_t res_row = 0;
    if (a.flags & F_RES_UP2) {
      const uint32_t ph = fd_div(rem, g.div_w);
      const uint32_t pw = rem - ph * g.div_w.d;
      res_row = (size_t)n * g.res_img_stride + (size_t)((ph >> 1) * (g.Wp >> 1) + (pw >> 1)) * Nout;
    } else if (a.flags & F_RES) {
      res_row = (size_t)n * g.res_img_stride + (size_t)rem * Nout;
    }
    const size_t dst_row = (size_t)n * g.dst_img_stride + (size_t)rem * Nout;
#pragma unroll
    for (int i = 0; i < FQ; ++i) {
      const int q = q0 + (wq * FQ + i) * 16 + fg * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (q + e >= Nout) break;
        float x = acc[i][j][e];
        if (a.flags & F_BIAS) x += a.bias[q + e];
        if (a.flags & (F_RES | F_RES_UP2)) x += (float)((const __bf16*)g.res)[res_row + q + e];
        if (a.flags & F_RELU) x = fmaxf(x, 0.f);
        if (a.flags & F_MASK) x = ((float)((const __bf16*)g.mask)[dst_row + q + e] > 0.f) ? x : 0.f;
        if (OUT_F32) ((float*)g.dst)[dst_row + q + e] = x;
        else ((__bf16*)g.dst)[dst_row + q + e] = (__bf16)x;
      }
    }
  }
}

// KP = pixels per K-step: 64 (two resident workgroups per CU) or 32 (half the LDS: three to four per CU, which is what the
// latency of the transposing ds_read_b64_tr_b16 fragment reads wants - they need more waves per SIMD than ds_read_b128).
// inline-asm transposing LDS read: invisible to hipcc's memory model, so it does not put a vmcnt(0) in front of it while LDS-DMA
// loads of OTHER ring slots are in flight (the builtin form does).  The caller waits lgkmcnt(0) + sched_barrier(0) before any use.
template <int OFF>
__device__ __forceinline__ s16x4_t lds_tr_read_asm(uint32_t addr) {
  s16x4_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

template <int KP, int NSTAGE>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const WgradArgs a) {
  constexpr int TILE = KP * 256, STAGE = 2 * TILE;   // [KP pixels][128 ch] bf16, two operands
  constexpr int NI = KP / 16;                        // staged rows per thread and operand
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int RS = a.R * a.S;
  const int tap = bid % RS; bid /= RS;
  const int ct = bid % a.CT; bid /= a.CT;
  const int qt = bid % a.QT; bid /= a.QT;
  const int z = bid;
  const int r = tap / a.S, s = tap - r * a.S;
  const int q0 = qt * 128, c0 = a.diag ? q0 : ct * 128;      // diag (grouped convolutions): the tile of the q-tile's own channels only
  const int Cdw = a.diag ? 128 : a.C, cd0 = a.diag ? 0 : c0;  // row length / first column of this tile in dw
  const int vbeg = z * a.v_per_split;
  int vend = vbeg + a.v_per_split; if (vend > a.V) vend = a.V;
  const int nsteps = (vend - vbeg) / KP;

  // staging: one wave instruction = 4 pixel rows x 256 B; lane -> (row_in, 16-B slot)
  const int srow = lane >> 4, spos = lane & 15;
  const int sswz = srow | (((wave >> 1) & 1) << 2);       // (row&3) | ((row>>3)&1)<<2, see header
  const int schunk = spos ^ (sswz << 1);                  // logical 16-B chunk (8 channels)
  const uint32_t qadd = (uint32_t)(q0 + schunk * 8) * 2u, cadd = (uint32_t)(c0 + schunk * 8) * 2u;
  const uint32_t qmask = (uint32_t) - (int)((q0 + schunk * 8) < a.K), cmask = (uint32_t) - (int)((c0 + schunk * 8) < a.C);

  // Level geometry lives in registers and is reloaded (wave-uniform branch) only when the virtual pixel index crosses
  // into the next level; stage() is called with increasing `it`.
  int cur_lv = 0;
#pragma unroll
  for (int i = 1; i < MAXLEV; ++i)
    if (i < a.nlev && vbeg >= a.lev[i].v0) cur_lv = i;
  WLevel g = a.lev[cur_lv];
  int next_v0 = (cur_lv + 1 < a.nlev) ? a.lev[cur_lv + 1].v0 : 0x7fffffff;
  auto yrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.dy), 0, g.dy_bytes, 0x00020000);
  auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.x), 0, g.x_bytes, 0x00020000);

  // Row state for the INCREMENTAL path (stride 1, "same" geometry, Wo >= 64): consecutive K-steps advance every row by 64
  // pixels, so (ho, wo) and both byte offsets are updated with a handful of adds/compares instead of two divisions and ~35
  // VALU per row and step (the wgrad loop was issue-bound: 113 M VALU against 67 M in the forward kernel for equal MFMAs).
  uint32_t r_oy[NI], r_ox[NI];
  int r_ho[NI], r_wo[NI], r_p[NI];
  bool fast = false;
  int dh = 0, dw = 0;
  uint32_t ycorr = 0, xcorr = 0;
  auto init_rows = [&](int pbase) {
    fast = (a.stride == 1) && (g.Wo >= KP) && (g.Ho == g.Hx) && (g.Wo == g.Wx);
    dh = r * a.dil - a.pad; dw = s * a.dil - a.pad;
    ycorr = (uint32_t)(g.dy_img_stride - g.Ho * g.Wo * a.K) * 2u;
    xcorr = (uint32_t)(g.x_img_stride - g.Hx * g.Wx * a.C) * 2u;
    const uint32_t tapshift = (uint32_t)((dh * g.Wx + dw) * a.C * 2);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (i * 4 + wave) * 4 + srow;
      const int p = pbase + row;
      const uint32_t n = fd_div((uint32_t)p, g.div_hw);
      const uint32_t rem = (uint32_t)p - n * g.div_hw.d;
      const uint32_t ho = fd_div(rem, g.div_w);
      const uint32_t wo = rem - ho * g.div_w.d;
      r_p[i] = p; r_ho[i] = (int)ho; r_wo[i] = (int)wo;
      r_oy[i] = (n * (uint32_t)g.dy_img_stride + rem * (uint32_t)a.K) * 2u + qadd;
      r_ox[i] = (n * (uint32_t)g.x_img_stride + rem * (uint32_t)a.C) * 2u + cadd + tapshift;
    }
  };
  init_rows(vbeg - g.v0);

  auto stage = [&](int it, char* buf) {
    const int v = vbeg + it * KP;
    if (v >= next_v0) {
      ++cur_lv;
      g = a.lev[cur_lv];
      next_v0 = (cur_lv + 1 < a.nlev) ? a.lev[cur_lv + 1].v0 : 0x7fffffff;
      yrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.dy), 0, g.dy_bytes, 0x00020000);
      xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.x), 0, g.x_bytes, 0x00020000);
      init_rows(v - g.v0);
    }
    if (fast) {
      const uint32_t ystep = (uint32_t)(2 * KP * a.K), xstep = (uint32_t)(2 * KP * a.C);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const bool pv = r_p[i] < g.P;
        const bool tv = ((unsigned)(r_ho[i] + dh) < (unsigned)g.Hx) & ((unsigned)(r_wo[i] + dw) < (unsigned)g.Wx);
        const uint32_t vy = (pv && qmask) ? r_oy[i] : SOD_OOB;
        const uint32_t vx = (pv && tv && cmask) ? r_ox[i] : SOD_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(yrsrc, SOD_LDS(buf + (i * 4 + wave) * 1024), 16, vy, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, SOD_LDS(buf + TILE + (i * 4 + wave) * 1024), 16, vx, 0, 0, 0);
        // advance this row by KP pixels (Wo >= KP: at most one column wrap and one image wrap)
        r_p[i] += KP; r_oy[i] += ystep; r_ox[i] += xstep;
        int wo = r_wo[i] + KP, ho = r_ho[i];
        if (wo >= g.Wo) { wo -= g.Wo; ho += 1; }
        if (ho >= g.Ho) { ho -= g.Ho; r_oy[i] += ycorr; r_ox[i] += xcorr; }
        r_wo[i] = wo; r_ho[i] = ho;
      }
      return;
    }
    const int pbase = v - g.v0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (i * 4 + wave) * 4 + srow;
      const int p = pbase + row;
      const uint32_t pm = (uint32_t) - (int)(p < g.P);
      const uint32_t pc = (uint32_t)p & pm;                      // clamp padding rows to pixel 0 (masked below)
      const uint32_t n = fd_div(pc, g.div_hw);
      const uint32_t rem = pc - n * g.div_hw.d;
      const uint32_t ho = fd_div(rem, g.div_w);
      const uint32_t wo = rem - ho * g.div_w.d;
      const uint32_t oy = (n * (uint32_t)g.dy_img_stride + rem * (uint32_t)a.K) * 2u + qadd;
      const int hi = (int)ho * a.stride - a.pad + r * a.dil;
      const int wi = (int)wo * a.stride - a.pad + s * a.dil;
      const uint32_t xm = (uint32_t) - (int)(((unsigned)hi < (unsigned)g.Hx) & ((unsigned)wi < (unsigned)g.Wx));
      const uint32_t ox = (n * (uint32_t)g.x_img_stride + ((uint32_t)hi * (uint32_t)g.Wx + (uint32_t)wi) * (uint32_t)a.C) * 2u + cadd;
      const uint32_t my = pm & qmask, mx = pm & cmask & xm;
      const uint32_t vy = (oy & my) | (SOD_OOB & ~my);
      const uint32_t vx = (ox & mx) | (SOD_OOB & ~mx);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yrsrc, SOD_LDS(buf + (i * 4 + wave) * 1024), 16, vy, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, SOD_LDS(buf + TILE + (i * 4 + wave) * 1024), 16, vx, 0, 0, 0);
    }
  };

  // transposed fragment reads: lane 4q+p of a 16-lane group addresses pixel row q, channels 4p..4p+3
  const int wq = wave >> 1, wc = wave & 1;
  const int tq = (lane & 15) >> 2, tp = lane & 3, tg = lane >> 4;
  const int tswz = tq | ((tg & 1) << 2);
  uint32_t aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    aoff[i] = (uint32_t)(8 * tg + tq) * 256u + (uint32_t)(((wq * 4 + i) ^ tswz) * 32) + tp * 8;
    boff[i] = TILE + (uint32_t)(8 * tg + tq) * 256u + (uint32_t)(((wc * 4 + i) ^ tswz) * 32) + tp * 8;
  }

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if constexpr (NSTAGE == 3) {
    // Three-slot LDS ring with a counted wait: the tile two K-steps ahead is requested while this one is computed, so a load has
    // two K-steps to land.  The split-over-pixels wgrad is latency-bound with a one-step prefetch (res4 conv2: 2 700 cycles per
    // 32-pixel step for 256 cycles of MFMA per wave, three workgroups per CU).  Every thread issues exactly LPS LDS-DMA loads per
    // stage() call, on every path.
    static_assert(KP == 32, "ring variant is built for 32-pixel steps");
    constexpr int LPS = NI * 2;
    const uint32_t lds0 = (uint32_t)(uintptr_t)SOD_LDS(smem);
    if (nsteps > 0) stage(0, smem);
    if (nsteps > 1) stage(1, smem + STAGE);
    int slot = 0;
    for (int it = 0; it < nsteps; ++it) {
      if (it + 1 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();   // tile `it` has landed for every wave; every wave has finished reading tile it-1
      const uint32_t cb = lds0 + (uint32_t)(slot * STAGE);
      s16x4_t alo[4], ahi[4], blo[4], bhi[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        alo[i] = lds_tr_read_asm<0>(cb + aoff[i]);
        ahi[i] = lds_tr_read_asm<1024>(cb + aoff[i]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        blo[j] = lds_tr_read_asm<0>(cb + boff[j]);
        bhi[j] = lds_tr_read_asm<1024>(cb + boff[j]);
      }
      int ns = slot + 2; if (ns >= 3) ns -= 3;
      if (it + 2 < nsteps) stage(it + 2, smem + ns * STAGE);   // overwrites the slot of tile it-1
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);                       // nothing that uses the fragments may move above the wait
      bf16x8_t af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s16x8_t v = {alo[i][0], alo[i][1], alo[i][2], alo[i][3], ahi[i][0], ahi[i][1], ahi[i][2], ahi[i][3]};
        af[i] = __builtin_bit_cast(bf16x8_t, v);
        s16x8_t w = {blo[i][0], blo[i][1], blo[i][2], blo[i][3], bhi[i][0], bhi[i][1], bhi[i][2], bhi[i][3]};
        bf[i] = __builtin_bit_cast(bf16x8_t, w);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
      slot = (slot == 2) ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
  if (nsteps > 0) stage(0, smem);
  for (int it = 0; it < nsteps; ++it) {
    char* cur = smem + (it & 1) * STAGE;
    __syncthreads();
    // ALL fragment reads of this K-step are issued BEFORE the next tile's LDS-DMA: hipcc puts an s_waitcnt vmcnt(0) in front of a
    // ds_read_b64_tr_b16 that follows an outstanding LDS-DMA (it cannot tell the two LDS ranges apart), which drained the prefetch
    // before the MFMAs and left only inter-workgroup overlap.  In this order the wait falls right after the barrier's own vmcnt(0).
    constexpr int KS = KP / 32;
    bf16x8_t af[KS][4], bf[KS][4];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)SOD_LDS(cur + aoff[i] + ks * 8192));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)SOD_LDS(cur + aoff[i] + ks * 8192 + 1024));
        s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        af[ks][i] = __builtin_bit_cast(bf16x8_t, v);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)SOD_LDS(cur + boff[j] + ks * 8192));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)SOD_LDS(cur + boff[j] + ks * 8192 + 1024));
        s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bf[ks][j] = __builtin_bit_cast(bf16x8_t, v);
      }
    }
    if (it + 1 < nsteps) stage(it + 1, smem + ((it + 1) & 1) * STAGE);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bf[ks][j], acc[i][j], 0, 0, 0);
  }
  }

  // D[row=q][col=c]
  const int fr = lane & 15, fg = lane >> 4;
  float* ptile = a.partial ? a.partial + ((size_t)z * (a.QT * a.CT * RS) + ((size_t)qt * a.CT + ct) * RS + tap) * (128 * 128) : nullptr;
  // The 16 per-row scale factors are fetched in one batch up front: a load inside the loop makes the compiler wait vmcnt(0) before
  // its use, and vmcnt also counts the atomics already in flight - every row then waited for all earlier (contended) atomics.
  float qsv[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + (wq * 4 + i) * 16 + fg * 4 + e;
      qsv[i][e] = (a.qscale && q < a.K) ? a.qscale[q] : 1.f;
    }
  if (!a.partial) {      // scale first (one wait for the batch of loads), so that nothing below depends on a load
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] *= qsv[i][e];
  }
  const int mode = a.partial ? 0 : (a.dbg_plain_store ? 1 : 2);      // wave-uniform, hoisted out of the element loops
  if (mode == 2 && q0 + 128 <= a.K && c0 + 128 <= a.C) {             // full tile: 64 atomics in straight-line code
    float* d0 = a.dw + ((size_t)(q0 + wq * 64 + fg * 4) * RS + tap) * Cdw + cd0 + wc * 64 + fr;
    const size_t qstride = (size_t)RS * Cdw;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(d0 + (size_t)(i * 16 + e) * qstride + j * 16, acc[i][j][e]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + (wq * 4 + i) * 16 + fg * 4 + e;
      if (q >= a.K) continue;
      float* drow = a.dw + ((size_t)q * RS + tap) * Cdw;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + (wc * 4 + j) * 16 + fr;
        if (c < a.C) {
          if (mode == 2) atomicAdd(drow + (c - c0 + cd0), acc[i][j][e]);
          else if (mode == 0) ptile[((wq * 4 + i) * 16 + fg * 4 + e) * 128 + (wc * 4 + j) * 16 + fr] = acc[i][j][e];
          else drow[c - c0 + cd0] = acc[i][j][e];
        }
      }
    }
  }
}

// Second stage of the split-over-pixels weight gradient for shapes with FEW output tiles (many splits per tile): the splits'
// partial tiles are summed here instead of hammering one 64-KB tile with nz x 16 K global atomics (measured: 15-50 us per call).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradArgs a) {
  const int RS = a.R * a.S, tiles = a.QT * a.CT * RS;
  const long long total = (long long)tiles * 128 * 32;          // float4 columns
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i & 31), row = (int)((i >> 5) & 127);
    int t = (int)(i >> 12);
    const int tap = t % RS; t /= RS;
    const int ct = t % a.CT, qt = t / a.CT;
    const int q = qt * 128 + row, c = (a.diag ? 0 : ct * 128) + c4 * 4;      // diag: dw rows are the 128 window columns
    const int Cdw = a.diag ? 128 : a.C;
    if (q >= a.K || c >= Cdw) continue;
    const float* src = a.partial + ((size_t)(i >> 12) * 128 + row) * 128 + c4 * 4;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    // blockIdx.y = chunk of splits (keeps >= 512 workgroups in flight for 4-tile shapes); chunks meet in dw with one atomic each
    const int zc = (a.nz + (int)gridDim.y - 1) / (int)gridDim.y, z0 = (int)blockIdx.y * zc;
    const int z1 = min(a.nz, z0 + zc);
    for (int z = z0; z < z1; ++z) acc += *reinterpret_cast<const f32x4_t*>(src + (size_t)z * tiles * (128 * 128));
    const float qs = a.qscale ? a.qscale[q] : 1.f;
    float* dst = a.dw + ((size_t)q * RS + tap) * Cdw + c;
    if (a.det) {       // gridDim.y == 1: this thread owns the four elements, fixed summation order
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < Cdw) dst[e] += acc[e] * qs;
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < Cdw) atomicAdd(dst + e, acc[e] * qs);
  }
}

template <int MODE, bool GENERIC, int WQ, int WP, int FQ, int FP, bool OUT_F32, int BK = 64, int NSTAGE = 2>
int launch_conv(const ConvArgs& a0, hipStream_t st, int* variant) {
  constexpr int BQ = WQ * FQ * 16, BP = WP * FP * 16;
  ConvArgs a = a0;
  a.T = (a.Kred + BK - 1) / BK;
  a.div_cpt = make_fastdiv((uint32_t)(GENERIC ? a.Cred / 8 : a.Cred / BK));
  a.div_rs = make_fastdiv((uint32_t)(a.R * a.S));
  // K order (channel chunk outer, tap inner): consecutive K-steps re-read the same pixel rows shifted by one tap, i.e. lines the CU's vector
  // cache still holds.  Few output channels, where the pixel operand is all the traffic: box_pred fwd 0.223 -> 0.111 ms.  For the other
  // shapes it is worth 0-3 % (the 128 -> 128 3x3 of res3: 119.1 -> 115.8 us; tap-inner everywhere: 629.9 -> 632.5 img/s over three
  // alternating pairs, inside the noise) and it changes the fp32 summation order of every 3x3 convolution, which the bf16 whole-model tests
  // on random-init models are sensitive to (discrete ReLU / sampling events): not the default.
  a.tap_inner = conv_tap_inner(BQ <= 16 ? 1 : 0);
  a.nq_tiles = (a.Nout + BQ - 1) / BQ;
  int tiles = 0;
  for (int l = 0; l < a.nlev; ++l) {
    a.lev[l].tile0 = tiles;
    tiles += (a.lev[l].P - a.lev[l].pstart + BP - 1) / BP;
  }
  a.np_tiles = tiles;
  if (tiles == 0) return SOD_OK;
  const size_t lds_full = NSTAGE * (size_t)(BQ + BP) * BK * 2;
  // a single K-step needs no second staging buffer: a smaller footprint lets 4 blocks share a CU, which is what hides the
  // load->MFMA->store latency of the memory-bound 1x1 convolutions (C = 64)
  const size_t epi = (size_t)(WQ * WP) * (size_t)(FP / 2) * 16 * (FQ * 64 + 16);
  size_t lds = a.T == 1 ? (size_t)(BQ + BP) * BK * 2 : lds_full;
  if (lds < epi) lds = epi;
  *variant = BQ * 100000 + BP * 100 + BK + (GENERIC ? 1 : 0);
  constexpr auto kern = conv_igemm_kernel<MODE, GENERIC, WQ, WP, FQ, FP, OUT_F32, BK, NSTAGE>;
  const hipError_t e = sod_max_dynamic_lds_once<kern>((int)(lds_full > epi ? lds_full : epi));
  if (e != hipSuccess) return (int)e;
  SOD_LAUNCH(kern, dim3(a.nq_tiles * a.np_tiles), dim3(64 * WQ * WP), lds, st, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

template <int MODE, bool OUT_F32>
int launch_tile(const ConvArgs& a, ConvTile tile, bool generic, hipStream_t st, int* variant) {
  switch (tile) {
    case TILE_16x256:
      return generic ? launch_conv<MODE, true, 1, 4, 1, 4, OUT_F32>(a, st, variant) : launch_conv<MODE, false, 1, 4, 1, 4, OUT_F32>(a, st, variant);
    case TILE_64x256:
      return generic ? launch_conv<MODE, true, 1, 4, 4, 4, OUT_F32>(a, st, variant) : launch_conv<MODE, false, 1, 4, 4, 4, OUT_F32>(a, st, variant);
    case TILE_128x128:
      return generic ? launch_conv<MODE, true, 2, 2, 4, 4, OUT_F32>(a, st, variant) : launch_conv<MODE, false, 2, 2, 4, 4, OUT_F32>(a, st, variant);
    case TILE_64x256_K32:
      return generic ? SOD_EARG : launch_conv<MODE, false, 1, 4, 4, 4, OUT_F32, 32>(a, st, variant);
    case TILE_128x128_K32:
      return generic ? SOD_EARG : launch_conv<MODE, false, 2, 2, 4, 4, OUT_F32, 32>(a, st, variant);
    // remainder tiles of a split dispatch (conv_dispatch.hip): 2 x 2 waves of 2 x 2 / 2 x 4 MFMA blocks, 64-deep K-steps
    case TILE_64x64:
      return generic ? SOD_EARG : launch_conv<MODE, false, 2, 2, 2, 2, OUT_F32>(a, st, variant);
    case TILE_64x128:
      return generic ? SOD_EARG : launch_conv<MODE, false, 2, 2, 2, 4, OUT_F32>(a, st, variant);
    case TILE_64x64_R3:
      return generic ? SOD_EARG : launch_conv<MODE, false, 2, 2, 2, 2, OUT_F32, 64, 3>(a, st, variant);
    case TILE_COUNT: break;
  }
  return SOD_EARG;
}

}  // namespace

namespace sodconv {

int launch_conv128(const ConvArgs& a, int mode, bool out_f32, ConvTile tile, bool generic, hipStream_t st, int* variant) {
  if (mode == MODE_FWD) return out_f32 ? launch_tile<MODE_FWD, true>(a, tile, generic, st, variant) : launch_tile<MODE_FWD, false>(a, tile, generic, st, variant);
  if (out_f32) return SOD_EARG;      // data gradients are bf16
  return launch_tile<MODE_DGRAD, false>(a, tile, generic, st, variant);
}

int launch_wgrad128(WgradArgs& a, int cus, int splits, float* ws, long long ws_bytes, hipStream_t st) {
  const int tiles = a.QT * a.CT * a.R * a.S;
  // 32 pixels per K-step, three-slot LDS ring (48 KB, 131 VGPRs) for every shape.  In the training step the wgrad kernels run on the side
  // stream BESIDE the data-gradient kernels, so the LDS footprint counts as well as the stand-alone rate.  Last sweeps on the FCOS R50 step
  // (rounds 1 - 2): ring everywhere, 2 workgroups per CU 581.2 / 581.0 img/s, 3 per CU 576.1 / 575.2, 1: 564; 64-pixel steps with two
  // slots for the few-tile shapes 544-547 vs 550.8-551.5 (those variants left the tree in round 5).
  if (splits <= 0) {
    // ONE resident wave of blocks (2 per CU): measured on the head shape, 504 blocks run at 718 TFLOP/s where 1548 blocks
    // (3.02 waves -> a nearly empty 4th round, 3x the atomic traffic) run at 585.  At least 256 pixels per block.
    long long Ptot = 0;
    for (int l = 0; l < a.nlev; ++l) Ptot += a.lev[l].P;
    splits = 2 * cus / tiles;
    const int maxs = (int)((Ptot + 255) / 256);
    if (splits > maxs) splits = maxs;
    if (splits < 1) splits = 1;
  }
  int vps = (a.V + splits - 1) / splits;
  vps = (vps + 63) / 64 * 64;
  a.v_per_split = vps;
  a.nz = (a.V + vps - 1) / vps;
  a.div_s = make_fastdiv((uint32_t)a.S);
  a.dbg_plain_store = 0;
  // Deterministic mode: fp32 partial tiles in the workspace + wgrad_reduce_kernel, summed in a fixed order with plain read-modify-writes;
  // otherwise the blocks meet in dW with fp32 atomics (the two-stage form as an option measured 447.4 vs 447.5 img/s, round 1).
  const long long need = (long long)a.nz * tiles * 128 * 128 * (long long)sizeof(float);
  if (a.det) {
    if (!ws || need > ws_bytes) return SOD_EARG;      // deterministic mode never falls back to atomics
    a.partial = ws;
  } else {
    a.partial = nullptr;
  }
  SOD_LAUNCH((conv_wgrad_kernel<32, 3>), dim3(a.nz * tiles), dim3(256), 3 * 2 * 32 * 256, st, a);
  if (a.partial) {
    const int gx = (tiles * 128 * 32 + 255) / 256;
    int gy = (1024 + gx - 1) / gx;            // ~1024 workgroups in total
    if (gy > a.nz) gy = a.nz;
    if (gy < 1 || a.det) gy = 1;
    SOD_LAUNCH(wgrad_reduce_kernel, dim3(gx, gy), dim3(256), 0, st, a);
  }
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

int launch_wgrad_reduce(const WgradArgs& a, hipStream_t st) {
  const int gx = (a.QT * a.CT * a.R * a.S * 128 * 32 + 255) / 256;
  SOD_LAUNCH(wgrad_reduce_kernel, dim3(gx, 1), dim3(256), 0, st, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

}  // namespace sodconv
