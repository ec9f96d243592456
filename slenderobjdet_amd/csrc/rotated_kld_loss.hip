// Gaussian KL-divergence box loss of rotated box pairs: sod_rotated_kld_loss, the pair operator with the contract of
// sod_rotated_iou_loss / sod_rotated_giou_loss (rotated_iou_loss.hip).  The loss of one pair and its gradient are rkld_pair of
// gauss_box_loss.h, where the definition and the closed form are written down; "rotated_kld" on the pitched delta buffer and over rows is
// the RkldLoss policy of box_loss_policy.h, which calls the same function.
// A kernel of its own: the IoU losses' kernel owns the 48 KB of clipping points of rotated_iou.h, which this loss has no use for - its
// only LDS is the 16 bytes of the block reduction, so the occupancy is bounded by registers alone.  The skeleton is that kernel's: 256
// threads, a grid-stride loop, one pair per thread, the forward sum through the reduce workspace (no float atomics: a call is
// bit-reproducible).  Latency-bound fp32 work, no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "gauss_box_loss.h"

__global__ __launch_bounds__(256) void rotated_kld_loss_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long long P,
                                                               float* __restrict__ elem, float* __restrict__ part,
                                                               const float* __restrict__ gscale, float* __restrict__ d1) {
  __shared__ float red[4];
  float acc = 0.f;
  const float gs = gscale ? gscale[0] : 1.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    float a[5], b[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) { a[e] = b1[i * 5 + e]; b[e] = b2[i * 5 + e]; }
    float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float l = d1 ? rkld_pair<true>(a, b, g) : rkld_pair<false>(a, b, g);
    if (elem) elem[i] = l;
    acc += l;
    if (d1) {
#pragma unroll
      for (int e = 0; e < 5; ++e) d1[i * 5 + e] = g[e] * gs;
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0 && part) part[blockIdx.x] = acc;
}

}  // namespace

extern "C" int sod_rotated_kld_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                    const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  if (P < 0 || (P > 0 && (!boxes1 || !boxes2)) || (sum_out && !ws)) return SOD_EARG;      // P == 0: sum_out = 0, nothing else written
  hipStream_t st = (hipStream_t)stream;
  const int g = sod_nblk(P);
  SOD_LAUNCH(rotated_kld_loss_kernel, dim3(g), dim3(256), 0, st, boxes1, boxes2, P, elem_out, sum_out ? ws : nullptr, grad_scale, dboxes1);
  if (sum_out) SOD_LAUNCH(sod_finish_sums_kernel<>, dim3(1), dim3(256), 0, st, ws, g, 1, sum_out, 0);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
