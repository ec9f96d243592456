// Gaussian KL-divergence box loss of rotated box pairs: sod_rotated_kld_loss, the pair operator with the contract of
// sod_rotated_iou_loss / sod_rotated_giou_loss (rotated_iou_loss.hip).  The loss of one pair and its gradient are rkld_pair of
// gauss_box_loss.h, where the definition and the closed form are written down; "rotated_kld" on the pitched delta buffer and over rows is
// the RkldLoss policy of box_loss_policy.h, which calls the same function.
// An instantiation of the pair skeleton of pair_loss.h (256 threads, a grid-stride loop, one pair per thread, the forward sum through the
// reduce workspace) WITHOUT the 48 KB of clipping points the IoU losses' instantiations own, which this loss has no use for: its only LDS
// is the 16 bytes of the block reduction, so the occupancy is bounded by registers alone.  Latency-bound fp32 work, no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "gauss_box_loss.h"
#include "pair_loss.h"          // pair_loss_kernel, launch_pairs

struct RkldPair {
  static constexpr int W = 5;
  using Lds = void;
  static constexpr int LDS_PER_LANE = 0;
  static __device__ __forceinline__ float pair(const float* a, const float* b, float, void*, bool want_grad, float* g) {
    return want_grad ? rkld_pair<true>(a, b, g) : rkld_pair<false>(a, b, g);
  }
};

}  // namespace

extern "C" int sod_rotated_kld_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                    const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<RkldPair>(boxes1, boxes2, P, 0.f, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}
