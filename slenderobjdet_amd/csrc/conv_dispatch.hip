// Host side of the convolutions: which kernel a forward / data-gradient / weight-gradient call goes to, the knobs of that choice, the
// optional per-launch timing, and every sod_conv2d_* / sod_conv_* entry point of the C ABI.  No device code: the kernels and their plain
// launchers live in conv_igemm.hip, conv_igemm256.hip, conv_pw.hip, conv_ws3.hip and conv_wgrad*.hip (declared in conv_args.h).
#include "conv_args.h"
#include <stdlib.h>
#include <atomic>
#include <algorithm>

using namespace sodconv;

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  return cus;
}

namespace {

thread_local int g_last_variant = 0;   // kernel variant chosen by the last forward / data-gradient dispatch (sod_conv_last_variant)
thread_local int g_last_tail = 0;      // tile code of that dispatch's remainder launch, 0 = none (sod_conv_last_tail_variant)
thread_local bool g_plan_only = false; // sod_conv_plan: walk the dispatch rules, launch nothing
thread_local int g_plan_main_pt = 0;   // sod_conv_plan: 256-pixel tiles of the main launch of a split dispatch
thread_local int g_conv_reverse = 0;   // sod_conv_set_reverse: per calling thread (the forward thread and autograd's worker each bracket their own launches)

// Every dispatch knob.  Process-wide; the setters of the C ABI write the same fields.
struct ConvKnobs {
  int conv256 = -1;         // SOD_CONV256 (default 1), sod_conv_set_tile256: 0 off; 1 heuristic; 2 every supported shape; -1: re-read at the next dispatch
  int pw = -1;              // SOD_CONV_PW (default 1), sod_conv_set_pw: 0 off; 1 on; -1: re-read at the next dispatch
  int ws3 = -1;             // SOD_CONV_WS3 (default 1), sod_conv_set_ws3: 0 off; 1 large launches; 2 every supported shape; -1: re-read at the next dispatch
  int tail = -1;            // SOD_CONV_TAIL (default 1), sod_conv_set_tail_tile: remainder launch of a split dispatch - 0 the ordinary rules' tile; 1 tail_tile_for(); else a forced
                            // tile code; -1: re-read at the next dispatch
  int tail_split = -1;      // SOD_CONV_TAIL_SPLIT (default 0), sod_conv_set_tail_split: > 0 splits every 256-capable dispatch after that many pixel tiles (tests, tools)
  int wgrad256 = 1;         // SOD_WGRAD256, read once: 0 never; 1 per-shape rule; 2 every supported shape
  int wgrad9 = 1;           // SOD_WGRAD9, read once: likewise
  int wgrad9_min_kt = 24;   // SOD_WGRAD9_MIN_KT, read once
  int wgrad_variant = -1;   // sod_conv_set_wgrad_variant only: -1 = per-shape choice, 0 = conv_wgrad_kernel, > 0 = that variant of conv_wgrad_ring.hip
};
ConvKnobs& knobs() {
  const auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  static ConvKnobs k = [&] {
    ConvKnobs k0;
    k0.wgrad256 = env("SOD_WGRAD256", k0.wgrad256);
    k0.wgrad9 = env("SOD_WGRAD9", k0.wgrad9);
    k0.wgrad9_min_kt = env("SOD_WGRAD9_MIN_KT", k0.wgrad9_min_kt);
    return k0;
  }();
  if (k.conv256 < 0) k.conv256 = env("SOD_CONV256", 1);
  if (k.pw < 0) k.pw = env("SOD_CONV_PW", 1);
  if (k.ws3 < 0) k.ws3 = env("SOD_CONV_WS3", 1);
  if (k.tail < 0) k.tail = env("SOD_CONV_TAIL", 1);
  if (k.tail_split < 0) k.tail_split = env("SOD_CONV_TAIL_SPLIT", 0);
  return k;
}

// Optional in-library timing of the conv launches (sod_conv_prof_enable / _collect): one hipEvent pair per top-level dispatch,
// recorded on the launch stream right around the MAIN kernel (for a split dispatch the 256x256 launch; `frac` is its share of the
// output pixels), so that the durations are comparable with rocprofv3's per-kernel figures.  The list is process-wide: autograd runs
// the backward pass on its own thread, and its dispatches belong to the same step as the forward ones.  Slots are reserved with an
// atomic counter; the nesting depth (tail launches of a split dispatch) is a per-thread property.
struct ConvProf {
  hipEvent_t* ev = nullptr;
  int* variant = nullptr;
  int* mode = nullptr;
  float* frac = nullptr;
  hipEvent_t* tail_ev = nullptr;      // sod_conv_prof_enable(2): a second pair per row around the remainder launch of a split dispatch
  int* tail_variant = nullptr;        // 0 = the row's dispatch had no remainder launch
  char* tail_timed = nullptr;
  int cap = 0;
  std::atomic<int> n{0};
  std::atomic<int> on{0};
};
ConvProf g_prof;
thread_local int g_prof_depth = 0;
thread_local int g_prof_row = -1;     // row of this thread's last top-level dispatch (-1: not recorded)
inline int prof_begin(hipStream_t st) {
  ConvProf& p = g_prof;
  if (!p.on.load(std::memory_order_relaxed) || g_prof_depth || g_plan_only) return -1;
  g_prof_row = -1;
  const int i = p.n.fetch_add(1);
  if (i >= p.cap) { p.n.store(p.cap); return -1; }
  g_prof_row = i;
  p.tail_variant[i] = 0; p.tail_timed[i] = 0;
  (void)hipEventRecord(p.ev[2 * i], st);
  return i;
}
inline void prof_end(int i, hipStream_t st, int variant, float frac, int mode) {
  if (i < 0) return;
  ConvProf& p = g_prof;
  (void)hipEventRecord(p.ev[2 * i + 1], st);
  p.variant[i] = variant; p.frac[i] = frac; p.mode[i] = mode;
}
// launch() between the two events of one profile row.  `variant` is read after the launch (launch_conv128 reports its tile code).
template <typename F>
int timed(hipStream_t st, const int& variant, float frac, int mode, F launch) {
  const int pi = prof_begin(st);
  const int rc = launch();
  prof_end(pi, st, variant, frac, mode);
  return rc;
}

// ---- the remainder launch of a split dispatch ----
// A remainder of a few 256-pixel tiles leaves most CUs empty, so its launch lasts as long as ONE workgroup's K loop (or a few, where
// several share a CU): a smaller tile has fewer MFMAs and fragment reads per K-step, a deeper LDS ring hides more of the load latency of
// a lone workgroup, and the loop is shorter.  With k workgroups resident per CU one round of a launch measured us_fixed[k - 1] +
// K-steps * us_step[k - 1] microseconds (K-steps of 64; launch to end, so the fixed part holds the launch itself, prologue and epilogue).
// estimate = whole rounds of max_per_cu workgroups per CU + the last round with k = ceil(workgroups left / CUs); the smallest estimate wins, and a tile
// must beat the 128x128 tile by 5 % to replace it.
// Constants: tools/bench_conv_tails.py --calibrate on one MI355X, 2026-10-20 (profiles/conv_tails_before.txt, "calibration": the forward
// rows at 36 and 16 K-steps solved for the two terms; k from the rows whose workgroup count gives that k).
struct TailTileCost {
  ConvTile tile;
  int max_per_cu;
  float us_fixed[4], us_step[4];
};
constexpr TailTileCost kTailTiles[] = {
    {TILE_128x128, 2, {10.1f, 11.6f, 0.f, 0.f}, {0.590f, 0.815f, 0.f, 0.f}},
    {TILE_64x128, 3, {7.9f, 8.8f, 9.4f, 0.f}, {0.545f, 0.558f, 0.850f, 0.f}},
    {TILE_64x64, 4, {6.1f, 6.6f, 7.5f, 8.2f}, {0.473f, 0.478f, 0.485f, 0.630f}},
    {TILE_64x64_R3, 3, {5.8f, 6.2f, 6.8f, 0.f}, {0.338f, 0.393f, 0.565f, 0.f}},
};
bool tail_tile_from_code(int code, ConvTile* tile) {
  for (const TailTileCost& c : kTailTiles)
    if (conv_tail_tile_code(c.tile) == code) { *tile = c.tile; return true; }
  return false;
}
// lev_pixels: the pixels each level leaves to the remainder launch
ConvTile tail_tile_for(const long long* lev_pixels, int nlev, int Nout, int Kred, int cus) {
  ConvTile best = TILE_128x128;
  double best_us = 0.0;
  const int steps = (Kred + 63) / 64;
  for (const TailTileCost& c : kTailTiles) {
    const ConvTileShape s = conv_tile_shape(c.tile);
    long long blocks = 0;
    for (int l = 0; l < nlev; ++l) blocks += (lev_pixels[l] + s.BP - 1) / s.BP;
    blocks *= (Nout + s.BQ - 1) / s.BQ;
    if (blocks <= 0) return TILE_128x128;
    const auto round_us = [&](long long k) { return (double)c.us_fixed[k - 1] + steps * (double)c.us_step[k - 1]; };
    const long long per_round = (long long)c.max_per_cu * cus, left = blocks % per_round;
    const double us = (double)(blocks / per_round) * round_us(c.max_per_cu) + (left ? round_us((left + cus - 1) / cus) : 0.0);
    if (c.tile == TILE_128x128) best_us = us * 0.95;
    else if (us < best_us) { best = c.tile; best_us = us; }
  }
  return best;
}

int dispatch_conv(const ConvArgs& a, int mode, bool out_f32, hipStream_t st) {
  const bool generic = (a.Cred & 63) != 0 || a.R * a.S > 64;      // the linear path keeps one validity bit per tap in 64-bit masks
  const auto conv128_of = [&](const ConvArgs& args, ConvTile tile) {
    if (g_plan_only) { g_last_variant = conv_tile_code(tile, generic); return (int)SOD_OK; }
    return timed(st, g_last_variant, 1.f, mode, [&] { return launch_conv128(args, mode, out_f32, tile, generic, st, &g_last_variant); });
  };
  const auto conv128 = [&](ConvTile tile) { return conv128_of(a, tile); };
  if (!g_prof_depth) { g_last_tail = 0; g_plan_main_pt = 0; }
  if (a.cwin) {         // channel window: the window IS the 128-row q-tile of this variant; Cred = 128 -> never generic
    if (generic || a.nlev != 1 || (a.Nout & 127)) return SOD_EARG;
    return conv128(TILE_128x128);
  }
  const ConvKnobs& k = knobs();
  const int cus = device_cus();
  // persistent weight-stationary kernel (conv_pw.hip) for the expanding 1x1 convolutions; SOD_CONV_PW=0 / sod_conv_set_pw(0) disables it
  if (k.pw && pw_supported(a, mode, out_f32, cus)) {
    g_last_variant = 7001;
    if (g_plan_only) return SOD_OK;
    return timed(st, 7001, 1.f, mode, [&] { return launch_pw(a, mode, st); });
  }
  // persistent weight-stationary 3x3 kernel (conv_ws3.hip) for the 128 -> 128 convolutions of res3; SOD_CONV_WS3=0 disables it
  if (k.ws3 && ws3_supported(a, mode, out_f32, cus, k.ws3 == 2)) {
    g_last_variant = 7003;
    if (g_plan_only) return SOD_OK;
    return timed(st, 7003, 1.f, mode, [&] { return launch_ws3(a, mode, st); });
  }
  // 256x256 8-phase kernel (conv_igemm256.hip) for the large compute-bound shapes.  SOD_CONV256=0 disables it, =2 forces it for
  // every shape it supports (parity tests).
  bool any_start = false;
  for (int l = 0; l < a.nlev; ++l) any_start |= a.lev[l].pstart != 0;
  // Data gradients use the 256 kernel as well.  Beside the wgrad side stream the answer depends on what the wgrad blocks leave free:
  // with 3-4 small wgrad workgroups per CU the 128-KB workgroup rarely found a CU (490 vs 487.5 img/s in favour of 128x128); with two
  // ring workgroups per CU and the faster wgrad it wins 542.4 vs 536.0.
  if (k.conv256 && !any_start && !(a.flags & (F_WBITS | F_MASKBITS)) && conv256_supported(a, mode)) {
    const int nq = (a.Nout + 255) / 256;
    long long pt256 = 0;
    for (int l = 0; l < a.nlev; ++l) pt256 += (a.lev[l].P + 255) / 256;
    const long long b256 = pt256 * nq;
    const auto conv256 = [&](int max_pt_tiles, float frac) {
      g_last_variant = 256;
      if (g_plan_only) return (int)SOD_OK;
      return timed(st, 256, frac, mode, [&] { return launch_conv256(a, mode, out_f32, max_pt_tiles, st); });
    };
    // The first main_pt pixel tiles on the 256 kernel, the rest in a remainder launch of the 128x128-family kernel (knobs().tail).
    const auto split_after = [&](int main_pt) {
      long long ptot = 0;
      for (int l = 0; l < a.nlev; ++l) ptot += a.lev[l].P;
      g_plan_main_pt = main_pt;
      int rc = conv256(main_pt, (float)((double)main_pt * 256.0 / (double)ptot));     // main tiles are full 256-pixel tiles
      if (rc) return rc;
      ConvArgs tail = a;
      long long left[MAXLEV];
      for (int l = 0; l < tail.nlev; ++l) {
        const int tl = (tail.lev[l].P + 255) / 256;
        if (main_pt >= tl) { tail.lev[l].pstart = tail.lev[l].P; main_pt -= tl; }
        else { tail.lev[l].pstart = main_pt * 256; main_pt = 0; }
        left[l] = tail.lev[l].P - tail.lev[l].pstart;
      }
      ConvTile tile = TILE_128x128;
      if (k.tail == 1) tile = tail_tile_for(left, tail.nlev, a.Nout, a.Kred, cus);
      else if (k.tail != 0 && !tail_tile_from_code(k.tail, &tile)) return (int)SOD_EARG;
      // the remainder launch belongs to this dispatch: no profile row of its own; sod_conv_prof_enable(2) times it in the main launch's row
      ConvProf& p = g_prof;
      const int row = (!g_plan_only && !g_prof_depth && p.on.load(std::memory_order_relaxed) == 2) ? g_prof_row : -1;
      if (row >= 0) (void)hipEventRecord(p.tail_ev[2 * row], st);
      ++g_prof_depth;
      if (k.tail == 0 || (k.tail == 1 && tile == TILE_128x128)) {      // the ordinary rules' tile (128x128, or its BK = 32 form for long remainders)
        rc = dispatch_conv(tail, mode, out_f32, st);
        g_last_tail = g_last_variant;
      } else {
        rc = conv128_of(tail, tile);
        g_last_tail = conv_tail_tile_code(tile);
      }
      --g_prof_depth;
      if (row >= 0) {
        (void)hipEventRecord(p.tail_ev[2 * row + 1], st);
        p.tail_timed[row] = 1;
      }
      if (!g_plan_only && !g_prof_depth && g_prof_row >= 0 && p.on.load(std::memory_order_relaxed)) p.tail_variant[g_prof_row] = g_last_tail;
      g_last_variant = 256;      // whole rounds on the 256 kernel (+ a short remainder launch)
      return rc;
    };
    if (k.tail_split > 0 && pt256 > k.tail_split) return split_after(k.tail_split);      // tests, tools/bench_conv_tails.py
    if (k.conv256 == 2) return conv256(0, 1.f);
    // (thresholds swept in rounds 2 - 4, DESIGN.md section 4: contraction >= 1024 - 512 / 256 measured 587-588 / 575 vs 593 img/s -, at
    // least one full round of tiles, output-channel counts that are no multiple of 256 - RetinaNet's 720 class scores: the third q-tile
    // is 19 % empty - from 512 channels up)
    constexpr int min_rounds = 1, min_k = 1024;
    if (a.Nout >= 256 && ((a.Nout & 255) == 0 || a.Nout >= 512) && a.Kred >= min_k && b256 >= (long long)min_rounds * cus) {
      // Measured (16 x FPN levels, 256 -> 256 3x3): 1020-1040 TFLOP/s against 840-930 for the 128x128 kernel.  Shapes with barely more
      // than one round of tiles (res4 conv2: 263 tiles = one round + a 7-tile remainder launch) measured slower stand-alone but win in
      // the training step (545.8-546.3 vs 541.2-542.9 img/s), so one full round is enough.
      // One workgroup per CU: a partial last round of 256x256 tiles wastes up to a whole round.  Whole rounds go to the 256 kernel,
      // a remainder below half a round is computed by the 128x128 kernel (two workgroups per CU, 4x smaller tiles) instead
      // (P3 output conv, 4.1 rounds: 1035 -> 1075 TFLOP/s).  Round 5 re-measured the threshold on the step - remainders up to 50 / 30 /
      // 12 / 5 % of a round split off: 633.2 / 631.7 / 634.6 / 631.0 img/s, three alternating 100-step runs each - no difference.
      const long long full = b256 / cus * cus, rem = b256 - full;
      if (rem == 0 || rem * 2 >= (long long)cus || (full / nq) * nq != full) return conv256(0, 1.f);
      return split_after((int)(full / nq));
    }
  }
  // (Round 6 measured an 80(q) x 256(p) tile - one wave row of 5 x 4 MFMA blocks, BK = 32, three workgroups per CU - for the 80 class scores
  // instead of 128 x 128 with 37.5 % of the q-tile empty: 195-204 us against 170 us on the P3 level, 664.1 vs 665.4 img/s on the step.  These
  // convolutions are bound by the pixel operand's way into LDS, not by the matrix pipe; not kept.)
  if (a.Nout <= 16) return conv128(TILE_16x256);
  // BK = 32: 4 blocks per CU for the res2-sized convs, +0.3 % on the step
  if (a.Nout <= 64) return conv128(!generic && (a.Cred & 31) == 0 ? TILE_64x256_K32 : TILE_64x256);
  // BK = 32 halves the LDS footprint (4 resident blocks per CU instead of 2): measured better for the latency-/write-bound
  // cases - short contractions - and worse for the large compute-bound shapes (head 3x3: 820 vs 699 TFLOP/s).
  long long blocks = 0;
  for (int l = 0; l < a.nlev; ++l) blocks += (a.lev[l].P - a.lev[l].pstart + 127) / 128;
  blocks *= (a.Nout + 127) / 128;
  // Re-measured per shape after the epilogue fix (serial run, best of the two variants 19.4 vs 19.9 ms of conv per step): grids that fit
  // one round of two blocks per CU want BK = 64 (P5/P6 3x3: 44 vs 54 us); otherwise BK = 32 also wins for Kred <= 512 (the 512-channel
  // 1x1 convs: 276 vs 300 us) and for the 128-channel 3x3 convs.
  const bool use32 = !generic && (a.Cred & 31) == 0 && blocks > 512 &&
                     (a.Kred <= 512 || blocks <= 1024 || (a.Cred <= 128 && a.Kred <= 1152));
  // (Measured and removed in round 5: a 3 / 4 / 5-slot LDS ring for the 32-deep K-steps - 113 -> 117 / 114 / 114 us on res3 conv3, -30 %
  // where it halves the workgroups per CU - and a 128(q) x 256(p) 8-wave tile with a 3-slot ring, 717 vs 813 TFLOP/s on the head shape;
  // a 4-slot ring of 64-deep steps for the one-workgroup-per-CU grids of the FPN top (P6 / P7, 20 - 70 workgroups): 29.4 vs 28.1 us -
  // their 0.78 us per K-step is issue time of one wave per SIMD, not load latency.)
  return conv128(use32 ? TILE_128x128_K32 : TILE_128x128);
}

int out_size(int H, int pad, int dil, int R, int stride) { return (H + 2 * pad - dil * (R - 1) - 1) / stride + 1; }

int fill_common(ConvArgs& a, int nlev, int N, int Cred, int Nout, int R, int S, int stride, int pad, int dil) {
  if (nlev <= 0 || nlev > MAXLEV) return SOD_EARG;
  if (N <= 0 || Nout <= 0 || R <= 0 || S <= 0 || stride <= 0 || dil <= 0 || pad < 0) return SOD_EARG;
  if (Cred <= 0 || (Cred & 7)) return SOD_EARG;
  const unsigned long long wb = (unsigned long long)Nout * R * S * Cred * 2ull;
  if (wb >= 0x80000000ull) return SOD_ESIZE;
  a.nlev = nlev;
  a.w_bytes = (uint32_t)wb;
  a.N = N; a.Cred = Cred; a.Nout = Nout; a.Cpitch = Cred; a.cwin = 0;
  a.R = R; a.S = S; a.stride = stride; a.pad = pad; a.dil = dil;
  a.Kred = R * S * Cred; a.T = (a.Kred + 63) / 64;
  a.div_cpt = make_fastdiv((uint32_t)((Cred & 63) ? Cred / 8 : Cred / 64));
  a.div_s = make_fastdiv((uint32_t)S);
  a.div_stride = make_fastdiv((uint32_t)stride);
  return SOD_OK;
}

// source dims (Hs,Ws) with Cred channels; GEMM-row dims (Hp,Wp) with Nout channels
int fill_level(ConvArgs& a, int l, const void* src, void* dst, int Hs, int Ws, int Hp, int Wp, long long src_img_stride,
               long long dst_img_stride, size_t dst_elt) {
  if (!src || !dst || Hs <= 0 || Ws <= 0 || Hp <= 0 || Wp <= 0) return SOD_EARG;
  if (src_img_stride <= 0) src_img_stride = (long long)Hs * Ws * a.Cpitch;
  if (dst_img_stride <= 0) dst_img_stride = (long long)Hp * Wp * a.Nout;
  if (src_img_stride < (long long)Hs * Ws * a.Cpitch || dst_img_stride < (long long)Hp * Wp * a.Nout) return SOD_EARG;
  const unsigned long long sb = (unsigned long long)a.N * src_img_stride * 2ull;
  const unsigned long long db = (unsigned long long)a.N * dst_img_stride * dst_elt;
  if (sb >= 0x80000000ull || db >= 0x200000000ull) return SOD_ESIZE;
  if ((long long)a.N * Hp * Wp >= (1ll << 31)) return SOD_ESIZE;
  LevelGeo& g = a.lev[l];
  g.src = src; g.dst = dst; g.res = nullptr; g.mask = nullptr; g.pstart = 0;
  g.src_bytes = (uint32_t)sb;
  g.Hs = Hs; g.Ws = Ws; g.Hp = Hp; g.Wp = Wp; g.P = a.N * Hp * Wp;
  g.src_img_stride = (int)src_img_stride; g.dst_img_stride = (int)dst_img_stride; g.res_img_stride = 0;
  g.div_hw = make_fastdiv((uint32_t)(Hp * Wp));
  g.div_w = make_fastdiv((uint32_t)Wp);
  return SOD_OK;
}

// Which kernel a weight gradient goes to.  SOD_WGRAD256: 0 = never, 1 (default) = shapes with K, C multiples of 256 whose blocks get
// at least 64 K-tiles of work each, 2 = every supported shape (parity tests).
bool use_wgrad256(const WgradArgs& a, float* ws, long long ws_bytes) {
  const int mode = knobs().wgrad256;
  // Blocks with few K-tiles are dominated by their 256-KB slab write, and the 48-KB workgroups of the 128x128 kernel share CUs with the
  // data-gradient kernels on the other stream.  Swept on the FCOS R50 step (one box, two rounds): >= 6 K-tiles per block 572.1 / 573.5
  // img/s, >= 40: 575.5 / 576.5, >= 70: 576.7 / 577.4, >= 120: 576.6 / 577.2, >= 250 (head towers off the 256 kernel): 565.6 / 566.1.
  // (re-swept with the faster kernel in round 4: 64 still best - 635.6 / 634.3 vs 633.2 at 32, 627-628 at 16 / 8)
  // (round 6, with the nine-tap kernel taking the long 3x3 shapes and the head's weight gradients parked behind the FPN backward: 32 beats 64 -
  // 663.9 / 662.5 / 664.6 vs 662.1 / 659.8 / 660.3 img/s, 20: 662.8 / 662.0 / 662.4; stand-alone the 256 kernel wins from ~30 K-tiles per block)
  constexpr int min_kt = 32;
  if (!mode || !ws || !wgrad256_supported(a)) return false;
  const int cus = device_cus();
  if (wgrad256_workspace_bytes(a, cus) > ws_bytes) return false;
  if (mode == 2) return true;
  // The kernel masks a partial last q-tile (K = 720 of RetinaNet's class scores: 27 tiles of which 9 are 19 % empty).  Until round 4 that
  // shape measured slower on it than on the 128x128 kernel (RetinaNet R50 527.5 / 527.1 vs 533.0 / 531.2 img/s); with the row arithmetic
  // out of the K loop it wins (546.6 / 548.5 vs 542.1 / 540.4; the 128x128 launch took 2.6 ms).
  long long V = 0;
  for (int l = 0; l < a.nlev; ++l) V += (a.lev[l].P + 63) / 64 * 64;
  const long long tiles = (long long)((a.K + 255) / 256) * (a.C / 256) * a.R * a.S;
  const long long nz = cus / tiles > 0 ? cus / tiles : 1;
  return V / 64 >= nz * min_kt;
}

// The nine-tap kernel (conv_wgrad9.hip) for the 3x3 convolutions it supports.  SOD_WGRAD9: 0 = never, 1 (default) = when every block gets
// at least `min_kt` K-tiles (prologue: ~E + 3 tile loads per level, epilogue: a 288-KB slab), 2 = every supported shape (parity tests).
bool use_wgrad9(const WgradArgs& a, float* ws, long long ws_bytes) {
  const int mode = knobs().wgrad9, min_kt = knobs().wgrad9_min_kt;
  if (!mode || !ws || !wgrad9_supported(a)) return false;
  const int cus = device_cus();
  if (wgrad9_workspace_bytes(a, cus) > ws_bytes) return false;
  return mode == 2 || wgrad9_tiles_per_block(a, cus) >= min_kt;
}

// Which variant of conv_wgrad_ring.hip a weight gradient takes (0 = conv_wgrad_kernel of conv_igemm.hip).
int ring_variant_for(const WgradArgs& a, int tiles, int splits, float* ws, long long ws_bytes) {
  const int v = knobs().wgrad_variant;
  if (a.diag) return 0;          // grouped convolutions: conv_wgrad_kernel's diagonal-tile mode only
  if (v >= 0) return v;
  // Measured per shape (tools/bench_wgrad_backbone.py, FCOS R50 at batch 16): the two groups of a workgroup halve the atomic bytes
  // (16 instead of 32 MB per launch: -9 ... -15 us on the 1x1 shapes of res3 / res4 / res5) but share one barrier per K-step, which costs
  // 3 - 9 % in long loops; the gain outweighs that up to ~100 K-steps per group.  Explicit split counts (tests) and deterministic mode
  // keep conv_wgrad_kernel and its slab reduce.
  if (splits != 0 || a.det || a.diag || tiles > 128) return 0;
  const int cus = device_cus();
  const long long steps = (long long)a.V / std::max(1, 2 * cus / tiles) / 32;
  return steps <= 100 ? 2300 : 0;
}

int dispatch_wgrad(WgradArgs& a, int splits, int flags, hipStream_t st, float* ws, long long ws_bytes) {
  const int cus = device_cus();
  a.det = (flags & WGRAD_DETERMINISTIC) ? 1 : 0;
  a.diag = (flags & WGRAD_DIAG) ? 1 : 0;
  if (a.diag && (a.C != a.K || (a.C & 127) || splits < 0)) return SOD_EARG;
  // splits == -2 forces the nine-tap kernel, -1 the 256 x 256 kernel (tests, tools); 0 = the dispatcher's choice
  if (splits == -2 && (!ws || !wgrad9_supported(a) || wgrad9_workspace_bytes(a, cus) > ws_bytes)) return SOD_EARG;
  if (splits == -2 || (splits == 0 && use_wgrad9(a, ws, ws_bytes)))
    return timed(st, 9009, 1.f, 2, [&] { return launch_wgrad9(a, cus, ws, ws_bytes, st); });
  if (splits == -1 && (!ws || !wgrad256_supported(a) || wgrad256_workspace_bytes(a, cus) > ws_bytes)) return SOD_EARG;
  if (splits == -1 || (splits == 0 && !a.diag && use_wgrad256(a, ws, ws_bytes)))
    return timed(st, 256, 1.f, 2, [&] { return launch_wgrad256(a, cus, ws, ws_bytes, st); });
  // few output channels (prediction convolutions): the taps folded into the tile rows, conv_wgrad_fold.hip
  if (splits == 0 && wgrad_fold_supported(a))
    return timed(st, 32004, 1.f, 2, [&] { return launch_wgrad_fold(a, cus, st); });
  a.QT = (a.K + 127) / 128; a.CT = a.diag ? 1 : (a.C + 127) / 128;
  const int tiles = a.QT * a.CT * a.R * a.S;
  int V = 0;
  long long Ptot = 0;
  for (int l = 0; l < a.nlev; ++l) {
    a.lev[l].v0 = V;
    V += (a.lev[l].P + 63) / 64 * 64;
    Ptot += a.lev[l].P;
  }
  a.V = V;
  // In-workgroup split over pixels with an LDS combine (conv_wgrad_ring.hip).  knobs().wgrad_variant: 0 = conv_wgrad_kernel, > 0 forces one
  // variant of launch_wgrad_ring for every shape, -1 (default) = the per-shape choice of ring_variant_for().
  const int variant = ring_variant_for(a, tiles, splits, ws, ws_bytes);
  if (variant > 0) {
    const int G = (variant % 10000) / 1000;      // + 10000 * ABL in ablation builds (conv_wgrad_ring.hip)
    int epi = (variant / 10) % 10;
    long long total = splits > 0 ? splits : (long long)G * std::max(1, (G == 1 ? 2 : 1) * cus / tiles);
    const long long maxs = (Ptot + 255) / 256;
    if (total > maxs) total = maxs;
    if (total < 1) total = 1;
    int vps = (int)((V + total - 1) / total);
    vps = (vps + 63) / 64 * 64;
    const int nsplit = (V + vps - 1) / vps;
    a.v_per_split = vps;
    a.nz = (nsplit + G - 1) / G;
    a.dbg_plain_store = 0;
    const long long need = (long long)a.nz * tiles * 128 * 128 * (long long)sizeof(float);
    if (a.det || epi == 1) {
      if (!ws || need > ws_bytes) {
        if (a.det) return SOD_EARG;
        epi = 0;
      }
    }
    a.partial = (a.det || epi == 1) ? ws : nullptr;
    const int v = variant - ((variant / 10) % 10) * 10 + (a.partial ? 10 : 0);
    return timed(st, v % 10000, 1.f, 2, [&] {          // G*1000 + NSTAGE*100 + EPI*10 + FDB (bench.py: kernel_name)
      const int rc = launch_wgrad_ring(a, v, st);
      return rc || !a.partial ? rc : launch_wgrad_reduce(a, st);
    });
  }
  return timed(st, 32003, 1.f, 2, [&] { return launch_wgrad128(a, cus, splits, ws, ws_bytes, st); });
}

int fill_wlevel(WgradArgs& a, int l, const void* dy, const void* x, int H, int W, long long dy_img_stride, long long x_img_stride) {
  if (!dy || !x || H <= 0 || W <= 0) return SOD_EARG;
  const int Ho = out_size(H, a.pad, a.dil, a.R, a.stride), Wo = out_size(W, a.pad, a.dil, a.S, a.stride);
  if (Ho <= 0 || Wo <= 0) return SOD_EARG;
  if (dy_img_stride <= 0) dy_img_stride = (long long)Ho * Wo * a.K;
  if (x_img_stride <= 0) x_img_stride = (long long)H * W * a.C;
  const unsigned long long yb = (unsigned long long)a.N * dy_img_stride * 2ull, xb = (unsigned long long)a.N * x_img_stride * 2ull;
  if (yb >= 0x80000000ull || xb >= 0x80000000ull || (long long)a.N * Ho * Wo >= (1ll << 30)) return SOD_ESIZE;
  WLevel& g = a.lev[l];
  g.dy = dy; g.x = x; g.dy_bytes = (uint32_t)yb; g.x_bytes = (uint32_t)xb;
  g.Hx = H; g.Wx = W; g.Ho = Ho; g.Wo = Wo; g.P = a.N * Ho * Wo;
  g.dy_img_stride = (int)dy_img_stride; g.x_img_stride = (int)x_img_stride;
  g.div_hw = make_fastdiv((uint32_t)(Ho * Wo));
  g.div_w = make_fastdiv((uint32_t)Wo);
  return SOD_OK;
}

// ---- shared bodies of the entry points.  A single-level entry point passes arrays of one. ----

struct Geo {      // the geometry arguments every entry point has
  int N;
  const int *H, *W;      // per level: the INPUT side of the convolution (x / dx)
  int C, K, R, S, stride, pad, dil;
};

bool out_positive(const Geo& g, int l) {
  return out_size(g.H[l], g.pad, g.dil, g.R, g.stride) > 0 && out_size(g.W[l], g.pad, g.dil, g.S, g.stride) > 0;
}

struct FwdExtra {
  const void* res = nullptr;        // single level: residual added in the epilogue (half resolution with SOD_CONV_RES_UP2)
  long long res_img_stride = 0;
  void* relu_bits = nullptr;        // single level: 1-bit ReLU mask of the output (F_WBITS)
  float* gn_sums = nullptr;         // GroupNorm statistics of the output, [nlev][N][G][2], zeroed here
  int G = 0;
  long long x_img_stride = 0;
  bool reverse = false;
};

int conv_fwd(int nlev, const void* const* x, const void* w, const float* bias, void* const* y, const Geo& g, long long y_img_stride,
             int flags, int out_f32, const FwdExtra& e, void* stream) {
  ConvArgs a{};
  const bool cwin = (flags & SOD_CONV_CWIN) != 0;      // window = the q-tile's own 128 channels; weights [K][R*S][128]
  int rc = fill_common(a, nlev, g.N, cwin ? 128 : g.C, g.K, g.R, g.S, g.stride, g.pad, g.dil);
  if (rc) return rc;
  if (cwin) { a.Cpitch = g.C; a.cwin = 1; }
  for (int l = 0; l < nlev; ++l) {
    if (!out_positive(g, l)) return SOD_EARG;
    rc = fill_level(a, l, x[l], y[l], g.H[l], g.W[l], out_size(g.H[l], g.pad, g.dil, g.R, g.stride), out_size(g.W[l], g.pad, g.dil, g.S, g.stride),
                    e.x_img_stride, y_img_stride, out_f32 ? 4 : 2);
    if (rc) return rc;
    if (e.gn_sums) a.lev[l].gn_sum = e.gn_sums + (size_t)l * g.N * e.G * 2;
  }
  a.w = w; a.bias = bias;
  a.gn_G = e.G;
  a.flags = (bias ? F_BIAS : 0) | ((flags & SOD_CONV_RELU) ? F_RELU : 0) | (e.gn_sums ? F_GNSTATS : 0);
  if (e.res) {
    LevelGeo& v = a.lev[0];
    v.res = e.res;
    if (flags & SOD_CONV_RES_UP2) {
      if ((v.Hp & 1) || (v.Wp & 1)) return SOD_EARG;
      a.flags |= F_RES_UP2;
      v.res_img_stride = (int)(e.res_img_stride > 0 ? e.res_img_stride : (long long)(v.Hp / 2) * (v.Wp / 2) * g.K);
    } else {
      a.flags |= F_RES;
      v.res_img_stride = (int)(e.res_img_stride > 0 ? e.res_img_stride : v.dst_img_stride);
    }
  }
  if (e.relu_bits) { a.flags |= F_WBITS; a.lev[0].bits = e.relu_bits; }
  if (e.reverse) a.flags |= F_REVERSE;
  hipStream_t st = (hipStream_t)stream;
  if (e.gn_sums) {
    hipError_t err = hipMemsetAsync(e.gn_sums, 0, sizeof(float) * 2 * (size_t)g.N * e.G * nlev, st);
    if (err != hipSuccess) return (int)err;
  }
  return dispatch_conv(a, MODE_FWD, out_f32 != 0, st);
}

struct DgradExtra {
  const void* const* accum = nullptr;   // per level, dx's shape: added in the epilogue (before the ReLU backward)
  bool accum_even = false;              // accum is (N, H/2, W/2, C): the compact data gradient of a stride-2 1x1 consumer
  const void* const* mask = nullptr;    // per level: dx = mask > 0 ? dx : 0; bf16 like dx, or with mask_bits one bit per element
  bool mask_bits = false;
  int Cpitch = 0;                       // > 0: channels per dY pixel in memory, where that is not the contraction width
  bool cwin = false;
  long long dx_img_stride = 0;
  bool reverse = false;
};

// GEMM rows are the INPUT pixels (H,W); the gather source is dY (Ho,Wo,Kred); output channels = C.
int conv_dgrad(int nlev, const void* const* dy, const void* wt, void* const* dx, const Geo& g, long long dy_img_stride, const DgradExtra& e,
               void* stream) {
  ConvArgs a{};
  int rc = fill_common(a, nlev, g.N, g.K, g.C, g.R, g.S, g.stride, g.pad, g.dil);
  if (rc) return rc;
  if (e.Cpitch > 0) a.Cpitch = e.Cpitch;
  a.cwin = e.cwin ? 1 : 0;
  for (int l = 0; l < nlev; ++l) {
    if (!out_positive(g, l) || (e.accum && !e.accum[l]) || (e.mask && !e.mask[l])) return SOD_EARG;
    rc = fill_level(a, l, dy[l], dx[l], out_size(g.H[l], g.pad, g.dil, g.R, g.stride), out_size(g.W[l], g.pad, g.dil, g.S, g.stride), g.H[l], g.W[l],
                    dy_img_stride, e.dx_img_stride, 2);
    if (rc) return rc;
    LevelGeo& v = a.lev[l];
    if (e.accum) { v.res = e.accum[l]; v.res_img_stride = e.accum_even ? (g.H[l] / 2) * (g.W[l] / 2) * g.C : v.dst_img_stride; }
    if (e.mask) v.mask = e.mask[l];
  }
  a.w = wt; a.bias = nullptr;
  a.flags = (e.accum ? (e.accum_even ? F_RES_UP2 | F_RES_EVEN : F_RES) : 0) | (e.mask ? (e.mask_bits ? F_MASKBITS : F_MASK) : 0) |
            (e.reverse ? F_REVERSE : 0);
  return dispatch_conv(a, MODE_DGRAD, false, (hipStream_t)stream);
}

int conv_wgrad(int nlev, const void* const* dy, const void* const* x, float* dw, const float* qscale, const Geo& g, long long dy_img_stride,
               long long x_img_stride, int splits, int flags, void* ws, long long ws_bytes, void* stream) {
  if (!dy || !x || !dw || !g.H || !g.W || nlev <= 0 || nlev > MAXLEV || ws_bytes < 0 || ((uintptr_t)ws & 15)) return SOD_EARG;
  if (g.N <= 0 || g.C <= 0 || g.K <= 0 || (g.C & 7) || (g.K & 7) || g.R <= 0 || g.S <= 0 || g.stride <= 0 || g.dil <= 0 || g.pad < 0) return SOD_EARG;
  WgradArgs a{};
  a.nlev = nlev; a.dw = dw; a.qscale = qscale; a.N = g.N; a.C = g.C; a.K = g.K;
  a.R = g.R; a.S = g.S; a.stride = g.stride; a.pad = g.pad; a.dil = g.dil;
  for (int l = 0; l < nlev; ++l) {
    const int rc = fill_wlevel(a, l, dy[l], x[l], g.H[l], g.W[l], dy_img_stride, x_img_stride);
    if (rc) return rc;
  }
  return dispatch_wgrad(a, splits, flags, (hipStream_t)stream, (float*)ws, ws ? ws_bytes : 0);
}

}  // namespace

extern "C" int sod_conv2d_fwd(const void* x, const void* w, const float* bias, const void* res, void* y,
                              int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                              long long x_img_stride, long long y_img_stride, long long res_img_stride,
                              int flags, int out_f32, void* stream) {
  const Geo g{N, &H, &W, C, K, R, S, stride, pad, dil};
  if (!x || !w || !y || !out_positive(g, 0)) return SOD_EARG;
  if ((flags & SOD_CONV_CWIN) && (C != K || (C & 127))) return SOD_EARG;
  FwdExtra e;
  e.res = res; e.res_img_stride = res_img_stride; e.x_img_stride = x_img_stride; e.reverse = g_conv_reverse != 0;
  return conv_fwd(1, &x, w, bias, &y, g, y_img_stride, flags, out_f32, e, stream);
}

extern "C" int sod_conv2d_fwd_bits(const void* x, const void* w, const float* bias, const void* res, void* y, void* relu_bits,
                                   int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil, int flags, void* stream) {
  const Geo g{N, &H, &W, C, K, R, S, stride, pad, dil};
  if (!relu_bits || !x || !w || !y || (K & 7) || !out_positive(g, 0)) return SOD_EARG;      // bits follow the dense bf16 output
  if (flags & SOD_CONV_CWIN) return SOD_EARG;
  FwdExtra e;
  e.res = res; e.relu_bits = relu_bits; e.reverse = g_conv_reverse != 0;
  return conv_fwd(1, &x, w, bias, &y, g, 0, flags, 0, e, stream);
}

extern "C" int sod_conv2d_fwd_ml(int nlev, const void* const* x, const void* w, const float* bias, void* const* y,
                                 int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                 long long y_img_stride, int flags, int out_f32, void* stream) {
  if (!x || !w || !y || !H || !W) return SOD_EARG;
  return conv_fwd(nlev, x, w, bias, y, Geo{N, H, W, C, K, R, S, stride, pad, dil}, y_img_stride, flags & SOD_CONV_RELU, out_f32, FwdExtra{}, stream);
}

extern "C" int sod_conv2d_fwd_ml_gnsum(int nlev, const void* const* x, const void* w, const float* bias, void* const* y,
                                       int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                       long long y_img_stride, int flags, float* gn_sums, int G, void* stream) {
  if (!x || !w || !y || !H || !W || !gn_sums) return SOD_EARG;
  if (G <= 0 || K != G * 8) return SOD_EARG;          // a lane's 8 output channels must be exactly one group
  FwdExtra e;
  e.gn_sums = gn_sums; e.G = G;
  return conv_fwd(nlev, x, w, bias, y, Geo{N, H, W, C, K, R, S, stride, pad, dil}, y_img_stride, flags & SOD_CONV_RELU, 0, e, stream);
}

extern "C" int sod_conv2d_dgrad(const void* dy, const void* wt, const void* accum, const void* relu_mask, void* dx,
                                int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                                long long dy_img_stride, long long dx_img_stride, void* stream) {
  const Geo g{N, &H, &W, C, K, R, S, stride, pad, dil};
  if (!dy || !wt || !dx || !out_positive(g, 0)) return SOD_EARG;
  DgradExtra e;
  e.accum = accum ? &accum : nullptr; e.mask = relu_mask ? &relu_mask : nullptr;
  e.dx_img_stride = dx_img_stride; e.reverse = g_conv_reverse != 0;
  return conv_dgrad(1, &dy, wt, &dx, g, dy_img_stride, e, stream);
}

// Data gradient of a grouped convolution in window mode (see SOD_CONV_CWIN): wt_win is [C][R*S][128], row c holds, per tap, the weights
// towards the 128 output channels of c's own 128-channel tile.  C == K, multiples of 128.
extern "C" int sod_conv2d_dgrad_cwin(const void* dy, const void* wt_win, const void* relu_mask, void* dx,
                                     int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil, void* stream) {
  const Geo g{N, &H, &W, C, 128, R, S, stride, pad, dil};      // the contraction is the window's 128 channels of dY's K
  if (!dy || !wt_win || !dx || C != K || (C & 127) || !out_positive(g, 0)) return SOD_EARG;
  DgradExtra e;
  e.mask = relu_mask ? &relu_mask : nullptr; e.Cpitch = K; e.cwin = true;
  return conv_dgrad(1, &dy, wt_win, &dx, g, 0, e, stream);
}

extern "C" int sod_conv2d_dgrad_bits(const void* dy, const void* wt, const void* accum, int accum_even, const void* relu_bits, void* dx,
                                     int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil, void* stream) {
  const Geo g{N, &H, &W, C, K, R, S, stride, pad, dil};
  if (!dy || !wt || !dx || !relu_bits || (C & 7)) return SOD_EARG;
  if (accum_even && (!accum || (H & 1) || (W & 1))) return SOD_EARG;
  if (!out_positive(g, 0)) return SOD_EARG;
  DgradExtra e;
  e.accum = accum ? &accum : nullptr; e.accum_even = accum_even != 0;
  e.mask = &relu_bits; e.mask_bits = true;
  return conv_dgrad(1, &dy, wt, &dx, g, 0, e, stream);
}

extern "C" int sod_conv2d_dgrad_ml(int nlev, const void* const* dy, const void* wt, void* const* dx,
                                   int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                   long long dy_img_stride, void* stream) {
  if (!dy || !wt || !dx || !H || !W) return SOD_EARG;
  return conv_dgrad(nlev, dy, wt, dx, Geo{N, H, W, C, K, R, S, stride, pad, dil}, dy_img_stride, DgradExtra{}, stream);
}

extern "C" int sod_conv2d_dgrad_ml_mask(int nlev, const void* const* dy, const void* wt, const void* const* relu_mask, void* const* dx,
                                        int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                        long long dy_img_stride, void* stream) {
  if (!dy || !wt || !dx || !relu_mask || !H || !W) return SOD_EARG;
  DgradExtra e;
  e.mask = relu_mask;
  return conv_dgrad(nlev, dy, wt, dx, Geo{N, H, W, C, K, R, S, stride, pad, dil}, dy_img_stride, e, stream);
}

// sod_conv2d_dgrad_ml for dY rows of `Kpitch` channels contracted as Kp >= Kpitch channels per tap (Kp a multiple of 64): wt_pad is
// [C][R][S][Kp] with zero columns from Kpitch on; the 16-byte chunks of the K loop that lie past a pixel's last channel are requested out
// of range (zero fill), never read from the next pixel or from behind the buffer.  A contraction that is no multiple of 64 channels per tap
// (RetinaNet's 720 class scores) otherwise takes the per-chunk gather path of the 128x128 kernel; padded to 768 it runs on the linear K
// loops, i.e. on the 256x256 kernel for the tower-sized output.  stride 1 only.
extern "C" int sod_conv2d_dgrad_ml_kpitch(int nlev, const void* const* dy, const void* wt_pad, void* const* dx,
                                          int N, const int* H, const int* W, int C, int Kp, int Kpitch, int R, int S, int pad, int dil,
                                          long long dy_img_stride, void* stream) {
  if (!dy || !wt_pad || !dx || !H || !W || Kpitch <= 0 || (Kpitch & 7) || Kp < Kpitch || (Kp & 63)) return SOD_EARG;
  DgradExtra e;
  e.Cpitch = Kpitch;
  return conv_dgrad(nlev, dy, wt_pad, dx, Geo{N, H, W, C, Kp, R, S, 1, pad, dil}, dy_img_stride, e, stream);
}

// sod_conv2d_dgrad_ml whose epilogue adds accum[l] (bf16, dx[l]'s shape) to level l's result: the SECOND of two consumers of the same
// tensors (the two FCOS towers read the same FPN outputs, fcosv2.py:342-361; the objectness and anchor-delta convs of the RPN head read the
// same hidden tensor) leaves the sum of both data gradients in one pass; relu_mask (optional, per level): the post-ReLU tensors the sum is
// the gradient of - the ReLU backward is applied after the addition (dX = mask > 0 ? dX + accum : 0).
extern "C" int sod_conv2d_dgrad_ml_accum(int nlev, const void* const* dy, const void* wt, const void* const* accum, const void* const* relu_mask,
                                         void* const* dx, int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                         long long dy_img_stride, void* stream) {
  if (!dy || !wt || !dx || !accum || !H || !W) return SOD_EARG;
  DgradExtra e;
  e.accum = accum; e.mask = relu_mask;
  return conv_dgrad(nlev, dy, wt, dx, Geo{N, H, W, C, K, R, S, stride, pad, dil}, dy_img_stride, e, stream);
}

extern "C" int sod_conv2d_wgrad(const void* dy, const void* x, float* dw, const float* qscale,
                                int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                                long long dy_img_stride, long long x_img_stride, int splits, int flags,
                                void* ws, long long ws_bytes, void* stream) {
  return conv_wgrad(1, &dy, &x, dw, qscale, Geo{N, &H, &W, C, K, R, S, stride, pad, dil}, dy_img_stride, x_img_stride, splits, flags, ws, ws_bytes,
                    stream);
}

// Workspace that lets every shape of one launch take the slab path: one 256x256 fp32 partial tile per CU plus the rounding of the
// split count, doubled for grids of more than one round (tiles > CUs).
extern "C" long long sod_conv2d_wgrad_workspace_bytes(void) { return 160ll << 20; }

extern "C" int sod_conv2d_wgrad_ml(int nlev, const void* const* dy, const void* const* x, float* dw, const float* qscale,
                                   int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                                   long long dy_img_stride, int splits, int flags, void* ws, long long ws_bytes, void* stream) {
  return conv_wgrad(nlev, dy, x, dw, qscale, Geo{N, H, W, C, K, R, S, stride, pad, dil}, dy_img_stride, 0, splits, flags, ws, ws_bytes, stream);
}

extern "C" int sod_conv_last_variant(void) { return g_last_variant; }

extern "C" int sod_conv_last_tail_variant(void) { return g_last_tail; }

extern "C" int sod_conv_tail_tile_select(long long tail_pixels, int Nout, int Kred, int cus) {
  if (tail_pixels <= 0 || Nout <= 0 || Kred <= 0 || cus <= 0) return SOD_EARG;
  return conv_tail_tile_code(tail_tile_for(&tail_pixels, 1, Nout, Kred, cus));
}

extern "C" int sod_conv_plan(int mode, int nlev, int N, const int* H, const int* W, int C, int K, int R, int S, int stride, int pad, int dil,
                             int* tail_variant, int* main_pt_tiles) {
  if (!H || !W || nlev <= 0 || nlev > MAXLEV || (mode != MODE_FWD && mode != MODE_DGRAD)) return SOD_EARG;
  void* const dummy = (void*)(uintptr_t)256;      // never dereferenced: nothing is launched
  const void* src[MAXLEV];
  void* dst[MAXLEV];
  for (int l = 0; l < nlev; ++l) { src[l] = dummy; dst[l] = dummy; }
  const Geo g{N, H, W, C, K, R, S, stride, pad, dil};
  g_plan_only = true;
  const int rc = mode == MODE_FWD ? conv_fwd(nlev, src, dummy, nullptr, dst, g, 0, 0, 0, FwdExtra{}, nullptr)
                                  : conv_dgrad(nlev, src, dummy, dst, g, 0, DgradExtra{}, nullptr);
  g_plan_only = false;
  if (rc) return rc < 0 ? rc : SOD_EARG;
  if (tail_variant) *tail_variant = g_last_tail;
  if (main_pt_tiles) *main_pt_tiles = g_plan_main_pt;
  return g_last_variant;
}

extern "C" int sod_conv_prof_enable(int on) {
  ConvProf& p = g_prof;
  if (on && !p.ev) {
    constexpr int CAP = 8192;
    p.ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * CAP);
    p.variant = (int*)malloc(sizeof(int) * CAP);
    p.mode = (int*)malloc(sizeof(int) * CAP);
    p.frac = (float*)malloc(sizeof(float) * CAP);
    p.tail_variant = (int*)malloc(sizeof(int) * CAP);
    p.tail_timed = (char*)malloc(CAP);
    if (!p.ev || !p.variant || !p.mode || !p.frac || !p.tail_variant || !p.tail_timed) return SOD_EARG;
    for (int i = 0; i < 2 * CAP; ++i)
      if (hipEventCreate(&p.ev[i]) != hipSuccess) return SOD_EARG;
    p.cap = CAP;
  }
  if (on == 2 && !p.tail_ev) {      // the remainder launches' own event pairs: only for the tool that asks for them
    hipEvent_t* ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * p.cap);
    if (!ev) return SOD_EARG;
    for (int i = 0; i < 2 * p.cap; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) return SOD_EARG;
    p.tail_ev = ev;
  }
  p.on.store(on == 2 ? 2 : on ? 1 : 0);
  return SOD_OK;
}

extern "C" int sod_conv_prof_collect_tails(float* tail_ms, int* tail_variant, int max) {
  ConvProf& p = g_prof;
  const int have = p.n.load();
  const int n = have < max ? have : max;
  if (n > 0 && (!tail_ms || !tail_variant)) return SOD_EARG;
  for (int i = 0; i < n; ++i) {
    float t = 0.f;
    if (p.tail_timed[i] && p.tail_ev) {
      if (hipEventSynchronize(p.tail_ev[2 * i + 1]) != hipSuccess) return SOD_EARG;
      if (hipEventElapsedTime(&t, p.tail_ev[2 * i], p.tail_ev[2 * i + 1]) != hipSuccess) return SOD_EARG;
    }
    tail_ms[i] = t; tail_variant[i] = p.tail_variant[i];
  }
  return n;
}

extern "C" int sod_conv_prof_collect(float* ms, int* variant, float* frac, int* mode, int max) {
  ConvProf& p = g_prof;
  const int have = p.n.load();
  const int n = have < max ? have : max;
  if (n > 0 && (!ms || !variant || !frac || !mode)) return SOD_EARG;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(p.ev[2 * i + 1]) != hipSuccess) return SOD_EARG;
    float t = 0.f;
    if (hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]) != hipSuccess) return SOD_EARG;
    ms[i] = t; variant[i] = p.variant[i]; frac[i] = p.frac[i]; mode[i] = p.mode[i];
  }
  p.n.store(0);
  return n;
}

// the single-level forward / data-gradient launches that follow walk their tiles last to first (see F_REVERSE)
extern "C" int sod_conv_set_reverse(int on) {
  g_conv_reverse = on ? 1 : 0;
  return SOD_OK;
}

extern "C" int sod_conv_set_wgrad_variant(int variant) {
  if (variant < -1) return SOD_EARG;
  knobs().wgrad_variant = variant;
  return SOD_OK;
}

extern "C" int sod_conv_set_ws3(int mode) {
  if (mode < -1 || mode > 2) return SOD_EARG;
  knobs().ws3 = mode;
  return SOD_OK;
}

extern "C" int sod_conv_set_pw(int on) {
  if (on < -1 || on > 1) return SOD_EARG;
  knobs().pw = on;
  return SOD_OK;
}

extern "C" int sod_conv_set_tail_tile(int mode) {
  ConvTile t;
  if (mode < -1 || (mode > 1 && !tail_tile_from_code(mode, &t))) return SOD_EARG;
  knobs().tail = mode;
  return SOD_OK;
}

extern "C" int sod_conv_set_tail_split(int main_tiles) {
  if (main_tiles < -1) return SOD_EARG;
  knobs().tail_split = main_tiles;
  return SOD_OK;
}

extern "C" int sod_conv_set_tile256(int mode) {
  if (mode < -1 || mode > 2) return SOD_EARG;
  knobs().conv256 = mode;
  return SOD_OK;
}
