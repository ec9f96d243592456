// FCOSRepPoints support kernels (slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py): the parts of the model that neither the FCOS
// kernels (losses.hip) nor the RepPoints kernels (reppoints.hip) cover.  HBM / latency-bound fp32 and integer work over (N, L) rows:
//   * the per-level Scale on the point rows of offsets_init (:639, :660), a learnable scalar read from the device;
//   * offsets2ltrb (:709-745) + the box decode of forward (:222-234): nine points -> signed LTRB distances, the decoded box and the arg
//     indices the backward scatter needs;
//   * get_ground_truth's second half (:343-374) for the whole batch: pairwise_iou + Matcher(allow_low_quality_matches) of every image's
//     gt boxes against ITS OWN predicted init boxes, then class / LTRB labels - two launches for N images, no G x L matrix;
//   * the loss finalisation (:263-317) with all normalisers kept on the device (the reference reads four of them back with .item()).
// (The slender top-k assignment is fcos_assign_kernel<true, true> in losses.hip and the linear-LTRB decode a mode of fcos_decode_kernel
// in inference_ops.hip: both share their kernel with the existing entry point through a parameter.)
#include "common.h"
#include "../../include/slender_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ Scale (layers/scale.py:5-11)
__global__ __launch_bounds__(256) void rpd_scale_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale, float* __restrict__ y,
                                                            long long n) {
  const float s = scale[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = x[i] * s;
}

__global__ __launch_bounds__(256) void rpd_scale_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ scale, float* __restrict__ dx, long long n,
                                                            float* __restrict__ part) {
  __shared__ float red[4];
  const float s = scale[0];
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = dy[i];
    dx[i] = d * s;
    acc += d * x[i];
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------ points -> LTRB (:709-745, :222-234)
struct P2LArgs {
  const float* pts;     // (N, H*W, ld): channel 2k = x offset, 2k+1 = y offset of point k
  const float* add;     // optional second addend with the same layout (offsets_refine + offsets_init.detach(), :695-698)
  float* ltrb;          // level slice of (N, L, 4): (-min x, -min y, max x, max y) of the points times pt_stride
  float* boxes;         // optional level slice of (N, L, 4): (cx - l, cy - t, cx + r, cy + b), cx = w * loc_stride + loc_stride / 2
  unsigned* arg;        // level slice of (N, L): byte c = index of the point that produced distance c (packing of sod_points2bbox_fwd)
  long long out_img_stride, arg_img_stride;
  int N, H, W, ld, npts, loc_stride;
  float pt_stride;
};

__global__ __launch_bounds__(256) void p2l_fwd_kernel(const P2LArgs a) {
  const long long HW = (long long)a.H * a.W, total = HW * a.N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    const float* r = a.pts + i * a.ld;
    const float* q = a.add ? a.add + i * a.ld : nullptr;
    float xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    unsigned ixmin = 0, ixmax = 0, iymin = 0, iymax = 0;
    for (int k = 0; k < a.npts; ++k) {
      float vx = r[2 * k], vy = r[2 * k + 1];
      if (q) { vx += q[2 * k]; vy += q[2 * k + 1]; }
      const float x = vx * a.pt_stride, y = vy * a.pt_stride;
      if (k == 0) { xmin = xmax = x; ymin = ymax = y; }
      else {                                            // strict comparisons: of equal extrema the lowest point index wins
        if (x < xmin) { xmin = x; ixmin = k; }
        if (x > xmax) { xmax = x; ixmax = k; }
        if (y < ymin) { ymin = y; iymin = k; }
        if (y > ymax) { ymax = y; iymax = k; }
      }
    }
    const f32x4_t d = {xmin * -1.f, ymin * -1.f, xmax, ymax};
    *reinterpret_cast<f32x4_t*>(a.ltrb + n * a.out_img_stride + p * 4) = d;
    if (a.boxes) {
      const int h = (int)(p / a.W), w = (int)(p - (long long)h * a.W);
      const float cx = (float)(w * a.loc_stride + a.loc_stride / 2), cy = (float)(h * a.loc_stride + a.loc_stride / 2);
      const f32x4_t b = {cx - d[0], cy - d[1], cx + d[2], cy + d[3]};
      *reinterpret_cast<f32x4_t*>(a.boxes + n * a.out_img_stride + p * 4) = b;
    }
    if (a.arg) a.arg[n * a.arg_img_stride + p] = ixmin | (iymin << 8) | (ixmax << 16) | (iymax << 24);
  }
}

__global__ __launch_bounds__(256) void p2l_bwd_kernel(const P2LArgs a, const float* __restrict__ dltrb, float* __restrict__ dpts32,
                                                      __bf16* __restrict__ dpts16) {
  const long long HW = (long long)a.H * a.W, total = HW * a.N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    const f32x4_t d = *reinterpret_cast<const f32x4_t*>(dltrb + n * a.out_img_stride + p * 4);
    const unsigned ar = a.arg[n * a.arg_img_stride + p];
    const int j0 = 2 * (int)(ar & 255), j1 = 2 * (int)((ar >> 8) & 255) + 1, j2 = 2 * (int)((ar >> 16) & 255), j3 = 2 * (int)(ar >> 24) + 1;
    for (int j = 0; j < a.ld; ++j) {
      float v = 0.f;
      if (j == j0) v -= d[0];            // l = -min x, t = -min y
      if (j == j1) v -= d[1];
      if (j == j2) v += d[2];
      if (j == j3) v += d[3];
      v *= a.pt_stride;
      if (dpts32) dpts32[i * a.ld + j] = v;
      if (dpts16) dpts16[i * a.ld + j] = (__bf16)v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ refine targets (:343-374)
// pairwise_iou(gt boxes of image n, init boxes of image n) + Matcher([lo, hi], [l0, l1, l2], allow_low_quality_matches) for all images.
// The two passes are anchor_match1_kernel / anchor_match2_kernel of detection_ops.hip with the image as grid.y and the image's own
// candidate rows: the same pair_iou, the same "first maximum wins", the same per-gt best through atomicMax on the IoU's bit pattern (its
// result does not depend on the order), the same low-quality rule - matches, matcher labels and matched values are bit-identical to N
// calls of sod_anchor_match.  The second pass goes on to the labels: the matched gt's class (background where the matcher says 0 -
// matcher label -1 keeps the class, :356-357 only rewrites label 0), -1 on locations outside the image, the matched box as LTRB distances.
struct RtArgs {
  const float* gts;        // (sum G, 4) XYXY
  const int* classes;      // (sum G)
  const int* box_off;      // (N + 1)
  const float* cand;       // (N, L, 4) XYXY, every image its own
  const float* image_hw;   // (N, 2) height, width
  int N, L, K, nlev, max_gt, total_gt;
  int lvl_off[SOD_MAX_LEVELS + 1], lvl_w[SOD_MAX_LEVELS], lvl_stride[SOD_MAX_LEVELS];
  float lo, hi;
  int l0, l1, l2, low_quality;
  float* vals; int* matches; signed char* mlab;       // (N, L)
  int* cls; int* cls_bg;                              // (N, L): {-1, 0..K-1, K}; cls_bg (optional) = cls with -1 replaced by K
  float* ltrb;                                        // (N, L, 4)
  unsigned* gt_best;                                  // (total_gt) words, zeroed by the entry point
};

__device__ __forceinline__ int rt_count(const RtArgs& a, int n, int& g0) {
  g0 = a.box_off[n];
  int G = a.box_off[n + 1] - g0;
  if (G > a.max_gt) G = a.max_gt;                     // the entry point checked the host's counts; keeps LDS / workspace indices in range
  if (g0 < 0 || g0 + G > a.total_gt) G = 0;
  return G < 0 ? 0 : G;
}

__global__ __launch_bounds__(256) void rt_match1_kernel(const RtArgs a) {
  extern __shared__ unsigned lbest[];   // [max_gt]
  const int n = blockIdx.y;
  int g0;
  const int G = rt_count(a, n, g0);
  for (int g = threadIdx.x; g < G; g += 256) lbest[g] = 0u;
  __syncthreads();
  const float* gts = a.gts + (long long)g0 * 4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.L; i += gridDim.x * 256) {
    const long long o = (long long)n * a.L + i;
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = a.cand[o * 4 + e];
    float bv = -1.f; int bi = 0;
    for (int g = 0; g < G; ++g) {
      const float v = pair_iou(gts + g * 4, c);
      if (v > bv) { bv = v; bi = g; }            // first maximum wins (torch.max(dim=0))
      if (v > 0.f) atomicMax(&lbest[g], __float_as_uint(v));
    }
    a.vals[o] = G > 0 ? bv : 0.f;                // Matcher on an empty gt set: everything unmatched
    a.matches[o] = bi;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) atomicMax(&a.gt_best[g0 + g], lbest[g]);
}

__global__ __launch_bounds__(256) void rt_match2_kernel(const RtArgs a) {
  const int n = blockIdx.y;
  int g0;
  const int G = rt_count(a, n, g0);
  const float* gts = a.gts + (long long)g0 * 4;
  const float img_h = a.image_hw[n * 2], img_w = a.image_hw[n * 2 + 1];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.L; i += gridDim.x * 256) {
    const long long o = (long long)n * a.L + i;
    const float v = a.vals[o];
    int lab = (v < a.lo) ? a.l0 : ((v < a.hi) ? a.l1 : a.l2);
    if (a.low_quality && G > 0) {
      float c[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) c[e] = a.cand[o * 4 + e];
      for (int g = 0; g < G; ++g)
        if (pair_iou(gts + g * 4, c) == __uint_as_float(a.gt_best[g0 + g])) { lab = 1; break; }
    }
    if (G == 0) lab = a.l0;
    a.mlab[o] = (signed char)lab;
    int lv = 0;
    while (lv + 1 < a.nlev && i >= a.lvl_off[lv + 1]) ++lv;
    const int idx = i - a.lvl_off[lv], st = a.lvl_stride[lv];
    const int iy = idx / a.lvl_w[lv], ix = idx - iy * a.lvl_w[lv];
    const float x = (float)(ix * st + st / 2), y = (float)(iy * st + st / 2);
    int c = a.K;
    f32x4_t d = {0.f, 0.f, 0.f, 0.f};
    if (G > 0) {
      const int m = a.matches[o];
      if (lab != 0) c = a.classes[g0 + m];
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(gts + (long long)m * 4);
      d = f32x4_t{x - b[0], y - b[1], b[2] - x, b[3] - y};
    }
    if (x >= img_w || y >= img_h) c = -1;        // centers_invalid (:349-350, :358)
    a.cls[o] = c;
    if (a.cls_bg) a.cls_bg[o] = c < 0 ? a.K : c;
    *reinterpret_cast<f32x4_t*>(a.ltrb + o * 4) = d;
  }
}

// ------------------------------------------------------------------------------------------------ finalize (:263-317)
__global__ void rpd_finalize_kernel(const float* __restrict__ focal_sum, const float* __restrict__ iou_sum, const float* __restrict__ sl1_sum,
                                    const float* __restrict__ bce_sum, const float* __restrict__ stats3, const float* __restrict__ n_refine,
                                    float inv_world, float* __restrict__ out8) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float nr = fmaxf(n_refine[0] * inv_world, 1.f);       // refine_num_pos_avg_per_gpu
    const float ni = fmaxf(stats3[0] * inv_world, 1.f);         // init_num_pos_avg_per_gpu
    const float ss = stats3[1] * inv_world;                     // sum_topk_centerness_targets_avg_per_gpu
    out8[0] = focal_sum[0] / nr;
    out8[1] = ss > 0.f ? iou_sum[0] / ss : 0.f;                 // nothing selected: the reference divides 0 by 0
    out8[2] = sl1_sum[0] / fmaxf(1.f, nr);
    out8[3] = bce_sum[0] / ni;
    // d(loss) / d(sum) of the three terms whose backward kernels take one scalar; a constant 1 for the kernels that divide by a second one
    out8[4] = ss > 0.f ? 1.f / ss : 0.f;
    out8[5] = 1.f / fmaxf(1.f, nr);
    out8[6] = 1.f / ni;
    out8[7] = 1.f;
  }
}

}  // namespace

extern "C" int sod_level_scale_fwd(const float* x, const float* scale, float* y, long long n, void* stream) {
  if (!x || !scale || !y || n < 0) return SOD_EARG;
  if (n == 0) return SOD_OK;
  SOD_LAUNCH(rpd_scale_fwd_kernel, dim3(sod_nblk(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, scale, y, n);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_level_scale_bwd(const float* dy, const float* x, const float* scale, float* dx, long long n, float* dscale, float* ws,
                                   void* stream) {
  if (!dy || !x || !scale || !dx || !dscale || !ws || n < 0) return SOD_EARG;
  if (n == 0) return SOD_OK;
  hipStream_t st = (hipStream_t)stream;
  const int g = sod_nblk(n);
  SOD_LAUNCH(rpd_scale_bwd_kernel, dim3(g), dim3(256), 0, st, dy, x, scale, dx, n, ws);
  SOD_LAUNCH(sod_finish_sums_kernel<>, dim3(1), dim3(256), 0, st, ws, g, 1, dscale, 1);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

static int p2l_fill(P2LArgs& a, int ld, int N, int H, int W, int loc_stride, float point_stride, int num_points, long long out_img_stride,
                    long long arg_img_stride) {
  if (N <= 0 || H <= 0 || W <= 0 || num_points <= 0 || num_points > 255 || ld < 2 * num_points || loc_stride < 0) return SOD_EARG;
  a.N = N; a.H = H; a.W = W; a.ld = ld; a.npts = num_points; a.loc_stride = loc_stride; a.pt_stride = point_stride;
  a.out_img_stride = out_img_stride > 0 ? out_img_stride : (long long)H * W * 4;
  a.arg_img_stride = arg_img_stride > 0 ? arg_img_stride : (long long)H * W;
  if ((a.out_img_stride & 3) || a.out_img_stride < (long long)H * W * 4 || a.arg_img_stride < (long long)H * W) return SOD_EARG;
  return SOD_OK;
}

extern "C" int sod_points2ltrb_fwd(const float* pts, const float* add, int ld, int N, int H, int W, int loc_stride, float point_stride,
                                   int num_points, float* ltrb, float* boxes, long long out_img_stride, unsigned* argidx,
                                   long long arg_img_stride, void* stream) {
  if (!pts || !ltrb) return SOD_EARG;
  P2LArgs a{};
  int rc = p2l_fill(a, ld, N, H, W, loc_stride, point_stride, num_points, out_img_stride, arg_img_stride);
  if (rc) return rc;
  a.pts = pts; a.add = add; a.ltrb = ltrb; a.boxes = boxes; a.arg = argidx;
  SOD_LAUNCH(p2l_fwd_kernel, dim3(sod_nblk((long long)N * H * W, 8192)), dim3(256), 0, (hipStream_t)stream, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_points2ltrb_bwd(const float* dltrb, long long out_img_stride, const unsigned* argidx, long long arg_img_stride, int ld,
                                   int N, int H, int W, float point_stride, int num_points, float* dpts_f32, void* dpts_bf16, void* stream) {
  if (!dltrb || !argidx || (!dpts_f32 && !dpts_bf16)) return SOD_EARG;
  P2LArgs a{};
  int rc = p2l_fill(a, ld, N, H, W, 0, point_stride, num_points, out_img_stride, arg_img_stride);
  if (rc) return rc;
  a.arg = const_cast<unsigned*>(argidx);
  SOD_LAUNCH(p2l_bwd_kernel, dim3(sod_nblk((long long)N * H * W, 8192)), dim3(256), 0, (hipStream_t)stream, a, dltrb, dpts_f32, (__bf16*)dpts_bf16);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_fcos_rpd_refine_targets(const float* gt_boxes, const int* gt_classes, const int* box_offsets, int N, int total_gt, int max_gt,
                                           const float* candidates, const float* image_hw, int nlevels, const int* lvl_h, const int* lvl_w,
                                           const int* lvl_stride, int num_classes, float thr_lo, float thr_hi, int label_below,
                                           int label_between, int label_above, int allow_low_quality, float* matched_vals, int* matches,
                                           signed char* match_labels, int* cls_labels, int* cls_labels_bg, float* refine_ltrb,
                                           unsigned* gt_best_ws, void* stream) {
  if (!box_offsets || !candidates || !image_hw || !lvl_h || !lvl_w || !lvl_stride || !matched_vals || !matches || !match_labels || !cls_labels ||
      !refine_ltrb)
    return SOD_EARG;
  if (N <= 0 || N > 65535 || nlevels <= 0 || nlevels > SOD_MAX_LEVELS || num_classes <= 0 || total_gt < 0 || max_gt < 0 || max_gt > total_gt) return SOD_EARG;
  if (max_gt > 4096) return SOD_EARG;                        // the limit of sod_anchor_match: the per-gt best IoUs of an image sit in LDS
  if (total_gt > 0 && (!gt_boxes || !gt_classes || !gt_best_ws)) return SOD_EARG;
  RtArgs a{};
  a.gts = gt_boxes; a.classes = gt_classes; a.box_off = box_offsets; a.cand = candidates; a.image_hw = image_hw;
  a.N = N; a.K = num_classes; a.nlev = nlevels; a.max_gt = max_gt; a.total_gt = total_gt;
  long long off = 0;
  for (int l = 0; l < nlevels; ++l) {
    if (lvl_h[l] <= 0 || lvl_w[l] <= 0 || lvl_stride[l] <= 0) return SOD_EARG;
    a.lvl_off[l] = (int)off; a.lvl_w[l] = lvl_w[l]; a.lvl_stride[l] = lvl_stride[l];
    off += (long long)lvl_h[l] * lvl_w[l];
  }
  if (off * N >= (1ll << 29)) return SOD_ESIZE;
  for (int l = nlevels; l <= SOD_MAX_LEVELS; ++l) a.lvl_off[l] = (int)off;
  a.L = (int)off;
  a.lo = thr_lo; a.hi = thr_hi; a.l0 = label_below; a.l1 = label_between; a.l2 = label_above; a.low_quality = allow_low_quality;
  a.vals = matched_vals; a.matches = matches; a.mlab = match_labels; a.cls = cls_labels; a.cls_bg = cls_labels_bg; a.ltrb = refine_ltrb;
  a.gt_best = gt_best_ws;
  hipStream_t st = (hipStream_t)stream;
  if (total_gt > 0) {
    hipError_t e = hipMemsetAsync(gt_best_ws, 0, sizeof(unsigned) * total_gt, st);
    if (e != hipSuccess) return (int)e;
  }
  const int gx = sod_nblk(a.L, 2048);
  SOD_LAUNCH(rt_match1_kernel, dim3(gx, N), dim3(256), sizeof(unsigned) * (max_gt > 0 ? max_gt : 1), st, a);
  SOD_LAUNCH(rt_match2_kernel, dim3(gx, N), dim3(256), 0, st, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_fcos_rpd_finalize(const float* focal_sum, const float* iou_sum, const float* smoothl1_sum, const float* bce_sum,
                                     const float* stats3, const float* n_refine, float inv_world, float* out8, void* stream) {
  if (!focal_sum || !iou_sum || !smoothl1_sum || !bce_sum || !stats3 || !n_refine || !out8) return SOD_EARG;
  SOD_LAUNCH(rpd_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, focal_sum, iou_sum, smoothl1_sum, bce_sum, stats3, n_refine, inv_world,
             out8);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
