// The skeleton of the pair operators: two (P, W) float arrays -> per row i the loss elem[i] of the pair (b1[i], b2[i]), optionally the sum
// over the rows, optionally the gradient w.r.t. b1 scaled by gscale[0].  ONE kernel template holds it - 256 threads, a grid-stride loop,
// one pair per lane, the scaled store of the gradient, the forward sum through the reduce workspace (no float atomics: a call is
// bit-reproducible) -, and a pair policy supplies what happens at one pair:
//   SmoothL1Pair      sod_smooth_l1_loss      detection_ops.hip        W = 1, param = beta
//   GiouXyxyPair      sod_giou_loss_xyxy      detection_ops.hip        W = 4, param = eps
//   RotIouPair<HULL>  sod_rotated_iou_loss / sod_rotated_giou_loss     rotated_iou_loss.hip     W = 5, owns the clipping points
//   RkldPair          sod_rotated_kld_loss    rotated_kld_loss.hip     W = 5
// A policy has: W; Lds and LDS_PER_LANE (the element type and the per-lane count of an LDS array the kernel owns for it: the 24 P2 of
// rotated_iou.h's clipping, 48 KB a block; void and 0: no array, the only LDS is the 16 bytes of the block reduction); and
// pair(a, b, param, lds, want_grad, g) -> the loss of the pair of W-vectors a and b; if want_grad, the W gradients w.r.t. a go to g (zeros
// before).  lds is the lane's first element, the lane stride 256.  One instantiation serves forward, backward and both: it chooses on the
// elem / part / d1 pointers at run time.  The including file places this header inside its own anonymous namespace, after common.h.
#pragma once

template <class Pair>
__global__ __launch_bounds__(256) void pair_loss_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long long P, float param,
                                                        float* __restrict__ elem, float* __restrict__ part, const float* __restrict__ gscale,
                                                        float* __restrict__ d1) {
  constexpr int W = Pair::W;
  __shared__ float red[4];
  typename Pair::Lds* lds = nullptr;
  if constexpr (Pair::LDS_PER_LANE > 0) {
    __shared__ typename Pair::Lds lane_lds[Pair::LDS_PER_LANE * 256];
    lds = lane_lds + threadIdx.x;
  }
  float acc = 0.f;
  const float gs = gscale ? gscale[0] : 1.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    float a[W], b[W], g[W];
    if constexpr (W == 4) {
      const f32x4_t av = *reinterpret_cast<const f32x4_t*>(b1 + i * 4), bv = *reinterpret_cast<const f32x4_t*>(b2 + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[e] = av[e]; b[e] = bv[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) { a[e] = b1[i * W + e]; b[e] = b2[i * W + e]; }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) g[e] = 0.f;
    const float l = Pair::pair(a, b, param, lds, d1 != nullptr, g);
    if (elem) elem[i] = l;
    acc += l;
    if (d1) {
      if constexpr (W == 4) *reinterpret_cast<f32x4_t*>(d1 + i * 4) = f32x4_t{g[0] * gs, g[1] * gs, g[2] * gs, g[3] * gs};
      else {
#pragma unroll
        for (int e = 0; e < W; ++e) d1[i * W + e] = g[e] * gs;
      }
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0 && part) part[blockIdx.x] = acc;
}

// P == 0 is legal, with NULL inputs too: sum_out = 0 if asked, nothing else written.
template <class Pair>
int launch_pairs(const float* a, const float* b, long long P, float param, float* elem_out, float* sum_out, const float* grad_scale, float* da,
                 float* ws, void* stream) {
  if (P < 0 || (P > 0 && (!a || !b)) || (sum_out && !ws)) return SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  const int g = sod_nblk(P);
  SOD_LAUNCH(pair_loss_kernel<Pair>, dim3(g), dim3(256), 0, st, a, b, P, param, elem_out, sum_out ? ws : nullptr, grad_scale, da);
  if (sum_out) SOD_LAUNCH(sod_finish_sums_kernel<>, dim3(1), dim3(256), 0, st, ws, g, 1, sum_out, 0);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
