// The fused decode + box regression loss over ROWS, forward and backward, for the R-CNN heads' BBOX_REG_LOSS_TYPE "giou" (D = 4),
// "rotated_iou", "rotated_giou" and "rotated_kld" (D = 5): row i regresses from src[i] (a sampled proposal or a sampled anchor) towards gt[i], and its
// deltas are D columns of the ld-wide row i of pred.  Two row forms say which rows count and which columns hold the deltas:
//   SOD_ROWS_FRCNN  int32 labels; foreground = 0 <= label < K; columns [label * D, label * D + D)   (FastRCNNOutputLayers, class-specific)
//   SOD_ROWS_RPN    int8 labels in {-1, 0, 1}; foreground = label == 1; columns [0, D)               (RPN / RRPN, the gathered sampled rows)
// At a foreground row the kernel calls the policies of box_loss_policy.h - the code the RetinaNet kernels of retina_box_loss.hip call -,
// so the same numbers give the same bits in both.  The skeleton is that kernel's: 256 threads, a grid-stride loop, one row per thread, the
// 48 KB of clipping points only in the rotated IoU instantiations, the forward sum through the reduce workspace (no float atomics: a call is
// bit-reproducible).  Backward writes EVERY element of dpred (R, ld): a block first leaves the <= 256 x D scaled delta gradients of its
// rows in LDS, then its threads walk the rows' 256 * ld consecutive floats together (coalesced) and store the gradient where a column
// belongs to the row's class and zero elsewhere - other classes, pad columns [K * D, ld), non-foreground rows.
// Latency-bound fp32 work on a few hundred to a few thousand rows, no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"
#include "box_transform.h"
#include "box_pair_loss.h"
#include "gauss_box_loss.h"
#include "box_loss_policy.h"

// DecodeLossArgs as the policies read it - pred, target = gt (R, D), anchors = src (R, D), w, clampv - with R rows of pitch ld and
// num_classes = K; labels (int32) serves the Fast R-CNN rows, labels8 the RPN rows.  N = A = 1.
struct RowsArgs : DecodeLossArgs {
  const signed char* labels8;
};

constexpr int ROWS_MAX_LD = 1 << 20;      // 256 * ld stays far below 2^31, where fd_div is exact

template <class Loss, bool RPN, bool BWD>
__global__ __launch_bounds__(256) void rows_box_loss_kernel(const RowsArgs a, const FastDiv ldiv, float* __restrict__ part,
                                                            const float* __restrict__ grad_scale, float scale_mul, float* __restrict__ dpred) {
  constexpr int D = Loss::D;
  __shared__ float red[4];
  __shared__ float grow[BWD ? D * 256 : 1];      // [e][row of the block]: the scaled delta gradients
  __shared__ int col0[BWD ? 256 : 1];            // first column of the row's deltas; -1: not a foreground row
  P2* pts = nullptr;
  if constexpr (Loss::ROT_LDS) {
    __shared__ P2 rot_pts[24 * 256];      // 48 KB: the clipping's candidate points (see RotPtsLds)
    pts = rot_pts + threadIdx.x;
  }
  float acc = 0.f;
  const float sc = BWD ? grad_scale[0] * scale_mul : 0.f;
  const long long R = a.R;
  for (long long base = (long long)blockIdx.x * 256; base < R; base += (long long)gridDim.x * 256) {      // block-uniform: barriers inside
    const long long i = base + threadIdx.x;
    int c0 = -1;
    float g[D];
#pragma unroll
    for (int e = 0; e < D; ++e) g[e] = 0.f;
    if (i < R) {
      if constexpr (RPN) {
        if (a.labels8[i] == 1) c0 = 0;
      } else {
        const int lab = a.labels[i];
        if (lab >= 0 && lab < a.num_classes) c0 = lab * D;
      }
      if (c0 >= 0) Loss::template positive<BWD>(a, a.pred + i * a.pitch + c0, i, i, pts, acc, g);
    }
    if constexpr (BWD) {
#pragma unroll
      for (int e = 0; e < D; ++e) grow[e * 256 + threadIdx.x] = g[e] * sc;
      col0[threadIdx.x] = c0;
      __syncthreads();
      const long long left = R - base;
      const uint32_t n = (uint32_t)(left < 256 ? left : 256) * (uint32_t)a.pitch;
      float* out = dpred + base * a.pitch;
      for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint32_t rl = fd_div(e, ldiv);
        const int k = (int)(e - rl * (uint32_t)a.pitch) - col0[rl];
        const bool own = col0[rl] >= 0 && k >= 0 && k < D;
        const float v = grow[(own ? k : 0) * 256 + rl];
        out[e] = own ? v : 0.f;
      }
      __syncthreads();      // the next round of the loop overwrites grow / col0
    }
  }
  if (!BWD) {
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
}

template <class Loss, bool RPN>
int launch(const RowsArgs& a, float* sum_out, float* ws, const float* grad_scale, float scale_mul, float* dpred, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const FastDiv ldiv = make_fastdiv((uint32_t)a.pitch);
  if (sum_out) {
    const int g = sod_nblk(a.R);
    SOD_LAUNCH((rows_box_loss_kernel<Loss, RPN, false>), dim3(g), dim3(256), 0, st, a, ldiv, ws, nullptr, 0.f, nullptr);
    SOD_LAUNCH(sod_finish_sums_kernel<>, dim3(1), dim3(256), 0, st, ws, g, 1, sum_out, 0);
  } else {
    if (a.R == 0) return SOD_OK;
    SOD_LAUNCH((rows_box_loss_kernel<Loss, RPN, true>), dim3(sod_nblk(a.R, 4096)), dim3(256), 0, st, a, ldiv, nullptr, grad_scale, scale_mul,
               dpred);
  }
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

// forward: sum_out and ws; backward: grad_scale and dpred
int rows_box_loss(const float* pred, int ld, const void* labels, int row_form, int K, const float* src, const float* gt, int R, int kind,
                  const float* weights, float scale_clamp, float* sum_out, float* ws, const float* grad_scale, float scale_mul, float* dpred,
                  void* stream) {
  if (kind != SOD_BOX_LOSS_GIOU && kind != SOD_BOX_LOSS_ROTATED_IOU && kind != SOD_BOX_LOSS_ROTATED_GIOU && kind != SOD_BOX_LOSS_ROTATED_KLD)
    return SOD_EARG;
  if (row_form != SOD_ROWS_FRCNN && row_form != SOD_ROWS_RPN) return SOD_EARG;
  const int D = kind == SOD_BOX_LOSS_GIOU ? 4 : 5;
  if (row_form == SOD_ROWS_RPN) K = 1;
  if (R < 0 || K <= 0 || ld < 0 || ld > ROWS_MAX_LD || (long long)K * D > ld) return SOD_EARG;
  if (D == 4 && ld % 4) return SOD_EARG;      // the XYXY policy reads its four deltas as one 16-byte word
  if (R > 0 && (!pred || !labels || !src || !gt)) return SOD_EARG;
  RowsArgs a{};
  if (!fill_w5(a.w, weights, D)) return SOD_EARG;
  a.pred = pred; a.target = gt; a.anchors = src; a.clampv = scale_clamp;
  a.N = 1; a.A = 1; a.R = R; a.pitch = ld; a.num_classes = K;
  if (row_form == SOD_ROWS_RPN) a.labels8 = (const signed char*)labels;
  else a.labels = (const int*)labels;
  const bool rpn = row_form == SOD_ROWS_RPN;
  if (kind == SOD_BOX_LOSS_GIOU)
    return rpn ? launch<GiouLoss, true>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream)
               : launch<GiouLoss, false>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream);
  if (kind == SOD_BOX_LOSS_ROTATED_IOU)
    return rpn ? launch<RiouLoss, true>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream)
               : launch<RiouLoss, false>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream);
  if (kind == SOD_BOX_LOSS_ROTATED_GIOU)
    return rpn ? launch<RgiouLoss, true>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream)
               : launch<RgiouLoss, false>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream);
  return rpn ? launch<RkldLoss, true>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream)
             : launch<RkldLoss, false>(a, sum_out, ws, grad_scale, scale_mul, dpred, stream);
}

}  // namespace

extern "C" int sod_rows_box_loss_fwd(const float* pred, int ld, const void* labels, int row_form, int K, const float* src, const float* gt, int R,
                                     int kind, const float* weights, float scale_clamp, float* sum_out, float* ws, void* stream) {
  if (!sum_out || !ws) return SOD_EARG;
  return rows_box_loss(pred, ld, labels, row_form, K, src, gt, R, kind, weights, scale_clamp, sum_out, ws, nullptr, 0.f, nullptr, stream);
}

extern "C" int sod_rows_box_loss_bwd(const float* pred, int ld, const void* labels, int row_form, int K, const float* src, const float* gt, int R,
                                     int kind, const float* weights, float scale_clamp, const float* grad_scale, float scale_mul, float* dpred,
                                     void* stream) {
  if (!grad_scale || (R > 0 && !dpred)) return SOD_EARG;
  return rows_box_loss(pred, ld, labels, row_form, K, src, gt, R, kind, weights, scale_clamp, nullptr, nullptr, grad_scale, scale_mul, dpred,
                       stream);
}
