// Slender-object COCO box evaluation on device: the per-(image, category) greedy matching, the precision / recall accumulation
// and the ratio x area bucketed proposal-recall pass of slender_det/evaluation (cocoeval.py, coco_evaluation.py:283-417).
//
// Every division and product here is a single IEEE operation in the precision the reference uses (float64 for COCOeval,
// float32 for the recall pass); the Makefile's -ffp-contract=off keeps them from being fused.
#include "common.h"
#include "../../include/slender_hip.h"

#define COCO_MAX_T 16
#define COCO_MAX_A 8
#define COCO_MAX_M 8
#define COCO_MAX_R 128
#define COCO_LDS_IOU 1600       // doubles of the staged [D, G] IoU matrix of one segment (12.8 KB); larger segments use scratch
#define ACC_THREADS 256

struct CocoMatchParams {
  double iou_thr[COCO_MAX_T];
  double lo[COCO_MAX_A], hi[COCO_MAX_A];
};

struct CocoAccParams {
  double rec_thr[COCO_MAX_R];
  int max_dets[COCO_MAX_M];
};

// pycocotools bbIou on XYWH boxes: float64, a crowd gt divides by the detection's area
__device__ __forceinline__ double coco_iou64(double dx, double dy, double dw, double dh, const double* g, bool crowd) {
  const double w = fmin(dx + dw, g[0] + g[2]) - fmax(dx, g[0]);
  if (w <= 0) return 0.0;
  const double h = fmin(dy + dh, g[1] + g[3]) - fmax(dy, g[1]);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double da = dw * dh;
  const double u = crowd ? da : (da + g[2] * g[3]) - i;
  return i / u;
}

// One workgroup (one wave) per (category k, image i) segment s = k * num_img + i.  Lane t * A + a runs the greedy scan of
// evaluateImg for IoU threshold t and ratio range a; the per-detection results of all lanes are one ballot each.
__global__ __launch_bounds__(64) void coco_match_kernel(const int* __restrict__ gt_off, const double* __restrict__ gt_box,
                                                        const unsigned char* __restrict__ gt_crowd, const double* __restrict__ gt_ratio,
                                                        const int* __restrict__ dt_off, const float* __restrict__ dt_box, int num_img,
                                                        int max_det, int T, int A, CocoMatchParams p,
                                                        const long long* __restrict__ scratch_off, double* __restrict__ scratch,
                                                        unsigned long long* __restrict__ dt_matched, unsigned long long* __restrict__ dt_ignored,
                                                        int* __restrict__ npig) {
  __shared__ double s_iou[COCO_LDS_IOU];
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  const int g0 = gt_off[s], G = gt_off[s + 1] - g0;
  const int d0 = dt_off[s];
  const int D = min(dt_off[s + 1] - d0, max_det);
  if (G == 0 && D == 0) return;   // evaluateImg returns None: the segment takes no part in accumulate
  const int k = s / num_img;
  const bool active = lane < T * A;
  const int t = active ? lane / A : 0, a = active ? lane % A : 0;
  const double lo = p.lo[a], hi = p.hi[a];
  if (lane < A) {
    int c = 0;
    for (int g = 0; g < G; ++g) {
      const double r = gt_ratio[g0 + g];
      c += !(gt_crowd[g0 + g] || r < p.lo[lane] || r > p.hi[lane]);
    }
    if (c) atomicAdd(npig + k * A + lane, c);
  }
  if (D == 0) return;
  // IoUs [D, G] staged once for all lanes: LDS, or this segment's slot of the global scratch
  const bool in_lds = (long long)D * G <= COCO_LDS_IOU;
  double* iou = in_lds ? s_iou : scratch + scratch_off[s];
  for (int idx = lane; idx < D * G; idx += 64) {
    const int d = idx / G, g = idx - (idx / G) * G;
    const float* db = dt_box + 4 * (size_t)(d0 + d);
    iou[idx] = coco_iou64((double)db[0], (double)db[1], (double)db[2], (double)db[3], gt_box + 4 * (size_t)(g0 + g), gt_crowd[g0 + g] != 0);
  }
  __syncthreads();
  // matched-gt flags of this lane: one register word for G <= 64, else a bit row in the scratch slot after the IoUs
  unsigned long long taken0 = 0;
  unsigned long long* taken = nullptr;
  const int words = (G + 63) / 64;
  if (G > 64) {
    taken = (unsigned long long*)(scratch + scratch_off[s] + (size_t)max_det * G) + (size_t)lane * words;
    if (active)
      for (int w = 0; w < words; ++w) taken[w] = 0ull;
  }
  const double thr = fmin(p.iou_thr[t], 1.0 - 1e-10);
  for (int d = 0; d < D; ++d) {
    bool mt = false, ig = false;
    if (active) {
      double best = thr;
      int m = -1;
      bool m_ig = false;
      // the gts in stable order with the ignored ones last: the non-ignored pass, then (unless a real gt matched) the ignored pass
      for (int pass = 0; pass < 2 && !(m >= 0 && !m_ig); ++pass) {
        for (int g = 0; g < G; ++g) {
          const double r = gt_ratio[g0 + g];
          const bool crowd = gt_crowd[g0 + g] != 0;
          const bool gig = crowd || r < lo || r > hi;
          if (gig != (pass == 1)) continue;
          const bool tk = G > 64 ? ((taken[g >> 6] >> (g & 63)) & 1ull) : ((taken0 >> g) & 1ull);
          if (tk && !crowd) continue;
          const double v = iou[(size_t)d * G + g];
          if (v < best) continue;
          best = v;
          m = g;
          m_ig = gig;
        }
      }
      if (m >= 0) {
        mt = true;
        ig = m_ig;
        if (G > 64) taken[m >> 6] |= 1ull << (m & 63);
        else taken0 |= 1ull << m;
      } else {
        const float* db = dt_box + 4 * (size_t)(d0 + d);
        const double ar = (double)db[2] / (double)db[3];
        ig = ar < lo || ar > hi;
      }
    }
    const unsigned long long bm = __ballot(mt), bi = __ballot(ig);
    if (lane == 0) {
      dt_matched[d0 + d] = bm;
      dt_ignored[d0 + d] = bi;
    }
  }
}

// Inclusive block scan (ACC_THREADS threads) of one int per thread.
__device__ __forceinline__ int block_scan_incl(int v, int* buf) {
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < ACC_THREADS; o <<= 1) {
    const int add = threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
    __syncthreads();
    buf[threadIdx.x] += add;
    __syncthreads();
  }
  return buf[threadIdx.x];
}

// One workgroup per (category k, range a, maxDets m, IoU threshold t).  The category's detections come in the order of one
// stable sort by (category, -score) of the segment-ordered list; those of rank >= maxDets[m] in their segment are left out.
// Precision at recall threshold r is the suffix maximum of pr from the first position whose recall reaches it; positions
// are binned by the largest r their tp count reaches, so one pass with an LDS max per bin gives every suffix maximum.
__global__ __launch_bounds__(ACC_THREADS) void coco_accumulate_kernel(const int* __restrict__ cat_off, const long long* __restrict__ order,
                                                                      const float* __restrict__ score, const int* __restrict__ rank,
                                                                      const unsigned long long* __restrict__ dt_matched,
                                                                      const unsigned long long* __restrict__ dt_ignored,
                                                                      const int* __restrict__ npig_all, int K, int T, int A, int M, int R,
                                                                      CocoAccParams p, double* __restrict__ precision,
                                                                      double* __restrict__ recall, double* __restrict__ scores) {
  __shared__ int need[COCO_MAX_R];
  __shared__ unsigned long long binmax[COCO_MAX_R];
  __shared__ double ss[COCO_MAX_R];
  __shared__ int scan[ACC_THREADS];
  int b = blockIdx.x;
  const int t = b % T; b /= T;
  const int m = b % M; b /= M;
  const int a = b % A;
  const int k = b / A;
  const int npig = npig_all[k * A + a];
  if (npig == 0) return;      // no gt of category k in range a: precision / recall stay -1
  const int max_det = p.max_dets[m];
  const int bit = t * A + a;
  const double dn = (double)npig;
  if (threadIdx.x < R) {
    // the smallest tp count c with c / npig >= recThrs[r] (np.searchsorted side='left' on rc = tp / npig)
    const double thr = p.rec_thr[threadIdx.x];
    long long c = (long long)ceil(thr * dn);
    if (c < 0) c = 0;
    while (c > 0 && (double)(c - 1) / dn >= thr) --c;
    while ((double)c / dn < thr) ++c;
    need[threadIdx.x] = c > 0x7fffffff ? 0x7fffffff : (int)c;
    binmax[threadIdx.x] = 0ull;
    ss[threadIdx.x] = 0.0;
  }
  __syncthreads();
  const int beg = cat_off[k], end = cat_off[k + 1];
  int tp_carry = 0, fp_carry = 0, n_carry = 0;
  for (int base = beg; base < end; base += ACC_THREADS) {
    const int j = base + threadIdx.x;
    bool valid = false, tp = false, fp = false;
    float sc = 0.f;
    if (j < end) {
      const long long q = order[j];
      valid = rank[q] < max_det;
      if (valid) {
        const bool mt = (dt_matched[q] >> bit) & 1ull, ig = (dt_ignored[q] >> bit) & 1ull;
        tp = mt && !ig;
        fp = !mt && !ig;
        sc = score[q];
      }
    }
    const int packed = block_scan_incl((int)tp | ((int)fp << 10) | ((int)valid << 20), scan);
    const int tp_cum = tp_carry + (packed & 1023), fp_cum = fp_carry + ((packed >> 10) & 1023);
    const int pos = n_carry + ((packed >> 20) & 1023) - 1;
    if (valid) {
      const double pr = (double)tp_cum / (((double)fp_cum + (double)tp_cum) + 2.220446049250313e-16);
      int lo = 0, hi = R - 1;           // largest r with need[r] <= tp_cum (need[0] == 0)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (need[mid] <= tp_cum) lo = mid; else hi = mid - 1;
      }
      atomicMax(&binmax[lo], (unsigned long long)__double_as_longlong(pr));   // pr >= 0: bit order is value order
      if (pos == 0)
        for (int r = 0; r < R && need[r] == 0; ++r) ss[r] = (double)sc;
      if (tp) {
        int l = 0, h = R;               // first r with need[r] >= tp_cum
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (need[mid] < tp_cum) l = mid + 1; else h = mid;
        }
        for (int r = l; r < R && need[r] == tp_cum; ++r) ss[r] = (double)sc;
      }
    }
    const int last = scan[ACC_THREADS - 1];
    tp_carry += last & 1023;
    fp_carry += (last >> 10) & 1023;
    n_carry += (last >> 20) & 1023;
    __syncthreads();
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t strideR = (size_t)K * A * M;
    const size_t base = (((size_t)t * R) * K + k) * A * M + (size_t)a * M + m;
    unsigned long long run = 0ull;
    for (int r = R - 1; r >= 0; --r) {
      run = binmax[r] > run ? binmax[r] : run;
      const bool hit = need[r] <= tp_carry && n_carry > 0;
      precision[base + r * strideR] = hit ? __longlong_as_double((long long)run) : 0.0;
      scores[base + r * strideR] = ss[r];
    }
    recall[(((size_t)t * K + k) * A + a) * M + m] = n_carry ? (double)tp_carry / dn : 0.0;
  }
}

namespace {

#include "proposal_ar.h"

// XYWH boxes: detectron2 pairwise_iou on XYXY boxes rebuilt in float32 from XYWH (x2 = x + w); a gt's area is that of the rebuilt box
struct ArXywhBox {
  static constexpr int W = 4;
  static constexpr int STAGE_LANES = AR_THREADS;
  using Lds = void;
  static constexpr int LDS_PER_LANE = 0;
  static __device__ __forceinline__ float overlap(const float* d, const float* g, Lds*) {
    const float dx2 = d[0] + d[2], dy2 = d[1] + d[3], gx2 = g[0] + g[2], gy2 = g[1] + g[3];
    const float a1 = (dx2 - d[0]) * (dy2 - d[1]);
    const float a2 = (gx2 - g[0]) * (gy2 - g[1]);
    const float w = fmaxf(fminf(dx2, gx2) - fmaxf(d[0], g[0]), 0.f);
    const float h = fmaxf(fminf(dy2, gy2) - fmaxf(d[1], g[1]), 0.f);
    const float inter = w * h;
    return inter > 0.f ? inter / ((a1 + a2) - inter) : 0.f;
  }
  static __device__ __forceinline__ float area(const float* g) {
    const float gx2 = g[0] + g[2], gy2 = g[1] + g[3];
    return (gx2 - g[0]) * (gy2 - g[1]);
  }
};

}  // namespace

extern "C" long long sod_coco_match_scratch_doubles(int num_gts, int max_det) {
  if (num_gts < 0 || max_det < 0) return -1;
  if ((long long)num_gts * max_det <= COCO_LDS_IOU && num_gts <= 64) return 0;
  return (long long)max_det * num_gts + (num_gts > 64 ? 64LL * ((num_gts + 63) / 64) : 0);
}

extern "C" int sod_coco_match(const int* gt_off, const double* gt_box, const unsigned char* gt_crowd, const double* gt_ratio,
                              const int* dt_off, const float* dt_box, int num_seg, int num_img, int max_det, const double* iou_thr,
                              int T, const double* ranges, int A, const long long* scratch_off, double* scratch,
                              unsigned long long* dt_matched, unsigned long long* dt_ignored, int* npig, void* stream) {
  if (num_seg < 0 || num_img <= 0 || num_seg % num_img || max_det <= 0 || T <= 0 || A <= 0 || T > COCO_MAX_T || A > COCO_MAX_A ||
      T * A > 64 || !iou_thr || !ranges || !gt_off || !dt_off || !scratch_off || !npig)
    return SOD_EARG;
  if (num_seg == 0) return SOD_OK;
  CocoMatchParams p;
  for (int t = 0; t < T; ++t) p.iou_thr[t] = iou_thr[t];
  for (int a = 0; a < A; ++a) {
    p.lo[a] = ranges[2 * a];
    p.hi[a] = ranges[2 * a + 1];
  }
  SOD_LAUNCH(coco_match_kernel, dim3(num_seg), dim3(64), 0, (hipStream_t)stream, gt_off, gt_box, gt_crowd, gt_ratio, dt_off, dt_box,
             num_img, max_det, T, A, p, scratch_off, scratch, dt_matched, dt_ignored, npig);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_coco_accumulate(const int* cat_off, const long long* order, const float* score, const int* rank,
                                   const unsigned long long* dt_matched, const unsigned long long* dt_ignored, const int* npig, int K,
                                   int T, int A, const int* max_dets, int M, const double* rec_thr, int R, double* precision,
                                   double* recall, double* scores, void* stream) {
  if (K < 0 || T <= 0 || A <= 0 || M <= 0 || R <= 0 || T > COCO_MAX_T || A > COCO_MAX_A || T * A > 64 || M > COCO_MAX_M ||
      R > COCO_MAX_R || !max_dets || !rec_thr || !cat_off || !npig || !precision || !recall || !scores)
    return SOD_EARG;
  if (K == 0) return SOD_OK;
  CocoAccParams p;
  for (int r = 0; r < R; ++r) p.rec_thr[r] = rec_thr[r];
  for (int m = 0; m < M; ++m) p.max_dets[m] = max_dets[m];
  SOD_LAUNCH(coco_accumulate_kernel, dim3(K * A * M * T), dim3(ACC_THREADS), 0, (hipStream_t)stream, cat_off, order, score, rank,
             dt_matched, dt_ignored, npig, K, T, A, M, R, p, precision, recall, scores);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" long long sod_proposal_ar_scratch_floats(int num_gts, int limit) { return proposal_ar_scratch_floats(num_gts, limit); }

extern "C" int sod_proposal_ar(const int* gt_off, const float* gt_box, const int* gt_cls, const float* gt_ratio, const int* dt_off,
                               const long long* dt_order, const float* dt_box, const int* dt_cls, int num_img, int limit, int K1,
                               const float* thr, int T, const float* ratio_rng, int R, const float* area_rng, int A,
                               const long long* scratch_off, float* scratch, int* hits, int* counts, float* recalls, void* stream) {
  return launch_proposal_ar<ArXywhBox>(gt_off, gt_box, gt_cls, gt_ratio, dt_off, dt_order, dt_box, dt_cls, num_img, limit, K1, thr, T,
                                       ratio_rng, R, area_rng, A, scratch_off, scratch, hits, counts, recalls, stream);
}
