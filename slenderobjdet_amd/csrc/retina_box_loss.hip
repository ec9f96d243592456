// The fused RetinaNet box regression loss on the pitched delta buffer (anchor a of pixel p at p*pitch + a*D), forward and backward, for
// RetinaNet / AnchorHead (D = 4) and RotatedRetinaNet (D = 5).  ONE kernel template holds the skeleton - the grid-stride loop over the
// N*R anchors, the index arithmetic, "positive = 0 <= label != num_classes", the scaled store of the delta gradient, the two-stage
// reduction -, and a loss policy supplies what happens at a positive:
//   SmoothL1Loss<4>  sod_retina_box_loss_*    smooth-L1 against the matched deltas                         (BBOX_REG_LOSS_TYPE "smooth_l1")
//   SmoothL1Loss<5>  sod_retina_box5_loss_*   the same over five deltas
//   GiouLoss         sod_retina_giou_loss_*   Box2BoxTransform.apply_deltas, fvcore giou_loss against the matched gt box          ("giou")
//   RiouLoss         sod_retina_riou_loss_*   Box2BoxTransformRotated.apply_deltas, 1 - rotated IoU against the matched gt box    ("rotated_iou")
//   RgiouLoss        sod_retina_rgiou_loss_*  the same decode, 1 - IoU + (hull - union) / hull against the matched gt box         ("rotated_giou")
//   RkldLoss         sod_retina_rkld_loss_*   the same decode, 1 - 1 / (1 + ln(1 + KL(N_box || N_gt))) of the boxes' Gaussians    ("rotated_kld")
// A policy has: D; Args (BoxLossArgs plus its own fields); ROT_LDS (whether the kernel owns the 48 KB of clipping points of rotated_iou.h);
// and positive<BWD>(a, p, r, i, pts, acc, g): for the positive anchor i = n*R + r whose deltas start at p, add the loss to acc (in place:
// smooth-L1 adds element by element, and the running sum's bits depend on that) and, if BWD, write the D delta gradients to g (zeros before).
// The backward kernel writes EVERY element of every pixel's pitch-wide row of dpred, pad columns [A*D, pitch) included (zeros there and in
// the rows of non-positives).  Latency / HBM-bound fp32 work on a fraction of a percent of the anchors, no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"
#include "box_transform.h"
#include "box_pair_loss.h"
#include "gauss_box_loss.h"
#include "box_loss_policy.h"      // BoxLossArgs, DecodeLossArgs; GiouLoss, RiouLoss, RgiouLoss, RkldLoss (shared with rows_box_loss.hip)

struct SmoothL1Args : BoxLossArgs { float beta; };

template <int D_>
struct SmoothL1Loss {
  static constexpr int D = D_;
  static constexpr bool ROT_LDS = false;
  using Args = SmoothL1Args;
  template <bool BWD>
  static __device__ __forceinline__ void positive(const Args& a, const float* p, long long r, long long i, P2* pts, float& acc, float* g) {
    float x[D], t[D];
    if constexpr (D == 4) {
      const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(p), tv = *reinterpret_cast<const f32x4_t*>(a.target + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { x[e] = xv[e]; t[e] = tv[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < D; ++e) { x[e] = p[e]; t[e] = a.target[i * D + e]; }
    }
#pragma unroll
    for (int e = 0; e < D; ++e) {
      const float d = x[e] - t[e], ad = fabsf(d);
      if (a.beta < 1e-5f) { acc += ad; g[e] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
      else if (ad < a.beta) { acc += 0.5f * d * d / a.beta; g[e] = d / a.beta; }
      else { acc += ad - 0.5f * a.beta; g[e] = d > 0.f ? 1.f : -1.f; }
    }
  }
};


// T: storage type of the delta gradient (bf16 product path, float in the fp32 validation mode)
template <class Loss, bool BWD, typename T>
__global__ __launch_bounds__(256) void retina_box_loss_kernel(const typename Loss::Args a, float* __restrict__ part, const float* __restrict__ gnum,
                                                              const float* __restrict__ gden, T* __restrict__ dpred) {
  constexpr int D = Loss::D;
  __shared__ float red[4];
  P2* pts = nullptr;
  if constexpr (Loss::ROT_LDS) {
    __shared__ P2 rot_pts[24 * 256];      // 48 KB: the clipping's candidate points (see RotPtsLds)
    pts = rot_pts + threadIdx.x;
  }
  float acc = 0.f, npos = 0.f;
  const float sc = BWD ? gnum[0] / gden[0] : 0.f;
  const long long total = (long long)a.N * a.R, pix_per_img = a.R / a.A;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / a.R, r = i - n * a.R, px = r / a.A;
    const int an = (int)(r - px * a.A);
    const long long po = (n * pix_per_img + px) * a.pitch + an * D;
    const int lab = a.labels[i];
    const bool pos = lab >= 0 && lab != a.num_classes;
    float g[D];
#pragma unroll
    for (int e = 0; e < D; ++e) g[e] = 0.f;
    if (pos) {
      npos += 1.f;
      Loss::template positive<BWD>(a, a.pred + po, r, i, pts, acc, g);
    }
    if (BWD) {
#pragma unroll
      for (int e = 0; e < D; ++e) dpred[po + e] = (T)(g[e] * sc);
      if (an == a.A - 1) {              // the pixel's last anchor also clears the pad columns [A*D, pitch)
        for (int c = D; c < a.pitch - an * D; ++c) dpred[po + c] = (T)0.f;
      }
    }
  }
  if (!BWD) {
    acc = block_sum_256(acc, red);
    npos = block_sum_256(npos, red);
    if (threadIdx.x == 0) { part[blockIdx.x] = acc; part[SOD_RED + blockIdx.x] = npos; }
  }
}

// sums[0] = the loss summed over positives, sums[1] = number of positives; normalizer <- m*normalizer + (1-m)*max(npos,1)
__global__ void retina_finish_kernel(const float* __restrict__ part, int nblk, float* __restrict__ sums, float* __restrict__ normalizer,
                                     float momentum) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) { a += part[i]; b += part[SOD_RED + i]; }
  a = block_sum_256(a, red);
  b = block_sum_256(b, red);
  if (threadIdx.x == 0) {
    sums[0] = a; sums[1] = b;
    if (normalizer) normalizer[0] = momentum * normalizer[0] + (1.f - momentum) * fmaxf(b, 1.f);
  }
}

// the common fields, then the policy's own; false = refuse the call
bool fill(BoxLossArgs& a, int D, const float* pred, int pitch, const int* labels, const float* target, int N, int R, int A, int K) {
  if (!pred || !labels || !target || N <= 0 || R <= 0 || A <= 0 || R % A || pitch < A * D) return false;
  a.pred = pred; a.labels = labels; a.target = target; a.N = N; a.R = R; a.A = A; a.pitch = pitch; a.num_classes = K;
  return true;
}
bool fill(SmoothL1Args& a, int D, const float* pred, int pitch, const int* labels, const float* deltas, int N, int R, int A, int K, float beta) {
  a.beta = beta;
  return fill((BoxLossArgs&)a, D, pred, pitch, labels, deltas, N, R, A, K);
}
bool fill(DecodeLossArgs& a, int D, const float* pred, int pitch, const int* labels, const float* anchors, const float* gt, int N, int R, int A,
          int K, const float* weights, float clampv) {
  a.anchors = anchors; a.clampv = clampv;
  return anchors && fill_w5(a.w, weights, D) && fill((BoxLossArgs&)a, D, pred, pitch, labels, gt, N, R, A, K);
}

template <class Loss>
int launch_fwd(const typename Loss::Args& a, float* sums2, float* normalizer, float momentum, float* ws, void* stream) {
  if (!sums2 || !ws) return SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  const int g = sod_nblk((long long)a.N * a.R);
  SOD_LAUNCH((retina_box_loss_kernel<Loss, false, __bf16>), dim3(g), dim3(256), 0, st, a, ws, nullptr, nullptr, nullptr);
  SOD_LAUNCH(retina_finish_kernel, dim3(1), dim3(256), 0, st, ws, g, sums2, normalizer, momentum);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

template <class Loss, typename T>
int launch_bwd(const typename Loss::Args& a, const float* grad_num, const float* grad_den, T* dpred, void* stream) {
  if (!grad_num || !grad_den || !dpred) return SOD_EARG;
  SOD_LAUNCH((retina_box_loss_kernel<Loss, true, T>), dim3(sod_nblk((long long)a.N * a.R, 4096)), dim3(256), 0, (hipStream_t)stream, a, nullptr,
             grad_num, grad_den, dpred);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

}  // namespace

#define SMOOTH_L1_FILL(D) SmoothL1Args a{}; if (!fill(a, D, pred, pitch, gt_labels, gt_deltas, N, R, A, num_classes, beta)) return SOD_EARG
#define DECODE_FILL(D, w) DecodeLossArgs a{}; if (!fill(a, D, pred, pitch, gt_labels, anchors, matched_boxes, N, R, A, num_classes, w, scale_clamp)) return SOD_EARG

extern "C" int sod_retina_box_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                       int num_classes, float beta, float* sums2, float* normalizer, float momentum, float* ws, void* stream) {
  SMOOTH_L1_FILL(4);
  return launch_fwd<SmoothL1Loss<4>>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_box_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                       int num_classes, float beta, const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  SMOOTH_L1_FILL(4);
  return launch_bwd<SmoothL1Loss<4>>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_box_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                           int num_classes, float beta, const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  SMOOTH_L1_FILL(4);
  return launch_bwd<SmoothL1Loss<4>>(a, grad_num, grad_den, dpred, stream);
}

extern "C" int sod_retina_box5_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                        int num_classes, float beta, float* sums2, float* normalizer, float momentum, float* ws, void* stream) {
  SMOOTH_L1_FILL(5);
  return launch_fwd<SmoothL1Loss<5>>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_box5_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                        int num_classes, float beta, const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  SMOOTH_L1_FILL(5);
  return launch_bwd<SmoothL1Loss<5>>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_box5_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* gt_deltas, int N, int R, int A,
                                            int num_classes, float beta, const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  SMOOTH_L1_FILL(5);
  return launch_bwd<SmoothL1Loss<5>>(a, grad_num, grad_den, dpred, stream);
}

extern "C" int sod_retina_giou_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights4, float scale_clamp, float* sums2,
                                        float* normalizer, float momentum, float* ws, void* stream) {
  DECODE_FILL(4, weights4);
  return launch_fwd<GiouLoss>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_giou_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights4, float scale_clamp,
                                        const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  DECODE_FILL(4, weights4);
  return launch_bwd<GiouLoss>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_giou_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                            int N, int R, int A, int num_classes, const float* weights4, float scale_clamp,
                                            const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  DECODE_FILL(4, weights4);
  return launch_bwd<GiouLoss>(a, grad_num, grad_den, dpred, stream);
}

extern "C" int sod_retina_riou_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp, float* sums2,
                                        float* normalizer, float momentum, float* ws, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_fwd<RiouLoss>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_riou_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                        const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RiouLoss>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_riou_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                            int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                            const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RiouLoss>(a, grad_num, grad_den, dpred, stream);
}

extern "C" int sod_retina_rgiou_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                         int N, int R, int A, int num_classes, const float* weights5, float scale_clamp, float* sums2,
                                         float* normalizer, float momentum, float* ws, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_fwd<RgiouLoss>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_rgiou_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                         int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                         const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RgiouLoss>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_rgiou_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                             int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                             const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RgiouLoss>(a, grad_num, grad_den, dpred, stream);
}

extern "C" int sod_retina_rkld_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp, float* sums2,
                                        float* normalizer, float momentum, float* ws, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_fwd<RkldLoss>(a, sums2, normalizer, momentum, ws, stream);
}
extern "C" int sod_retina_rkld_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                        const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RkldLoss>(a, grad_num, grad_den, (__bf16*)dpred_bf16, stream);
}
extern "C" int sod_retina_rkld_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                            int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                            const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  DECODE_FILL(5, weights5);
  return launch_bwd<RkldLoss>(a, grad_num, grad_den, dpred, stream);
}
