// The decode-and-loss policies of the fused box losses: what happens at ONE positive whose deltas are decoded against the box it regresses
// from and compared with its matched gt box.  Two skeletons call them - retina_box_loss_kernel (retina_box_loss.hip: anchors of a pitched
// per-pixel delta buffer) and rows_box_loss_kernel (rows_box_loss.hip: rows of sampled ROIs / sampled anchors) -, so there is one
// definition of every loss and the two give the same bits for the same numbers.  The including file places this header inside its own
// anonymous namespace, after common.h, rotated_iou.h, box_transform.h, box_pair_loss.h and gauss_box_loss.h.
#pragma once

struct BoxLossArgs {
  const float* pred;        // (N, sumHW, pitch) fp32
  const int* labels;        // (N, R)
  const float* target;      // (N, R, D): the matched deltas (smooth-L1) or the matched gt boxes (the IoU losses)
  int N, R, A, pitch, num_classes;
};
struct DecodeLossArgs : BoxLossArgs {
  const float* anchors;     // (R, D)
  W5 w;
  float clampv;
};

// A policy has: D; Args (BoxLossArgs plus its own fields); ROT_LDS (whether the kernel owns the 48 KB of clipping points of rotated_iou.h);
// and positive<BWD>(a, p, r, i, pts, acc, g): for the positive whose deltas start at p, whose source box is row r of a.anchors and whose
// gt box is row i of a.target, add the loss to acc and, if BWD, write the D delta gradients to g (zeros before).

// retina_rotated.py:236-245; AnchorHead, meta/heads/anchor_head.py:366-374.  The clamp keeps a NaN delta (see ClampForm): the loss is NaN then.
struct GiouLoss {
  static constexpr int D = 4;
  static constexpr bool ROT_LDS = false;
  using Args = DecodeLossArgs;
  template <bool BWD>
  static __device__ __forceinline__ void positive(const Args& a, const float* p, long long r, long long i, P2* pts, float& acc, float* g) {
    const f32x4_t d = *reinterpret_cast<const f32x4_t*>(p), anc = *reinterpret_cast<const f32x4_t*>(a.anchors + r * 4);
    const f32x4_t gt = *reinterpret_cast<const f32x4_t*>(a.target + i * 4);
    float box[4], gb[4];
    const XyxyDecoded k = xyxy_apply_deltas<CLAMP_KEEPS_NAN>(d, anc, a.w.w, a.clampv, box);
    acc += giou_pair(box, gt, 1e-7f, BWD ? gb : nullptr);
    if (BWD) {
      g[0] = (gb[0] + gb[2]) * k.bw / a.w.w[0];
      g[1] = (gb[1] + gb[3]) * k.bh / a.w.w[1];
      g[2] = k.cw ? 0.f : (gb[2] - gb[0]) * 0.5f * k.pw / a.w.w[2];
      g[3] = k.ch ? 0.f : (gb[3] - gb[1]) * 0.5f * k.ph / a.w.w[3];
    }
  }
};

// The chain from the gradient gb w.r.t. the box that rot_apply_deltas decoded from source box s to the gradient g w.r.t. its five deltas
// (gb[4] per degree): d cx / d dx = sw / wx, d w / d dw = w / ww and 0 where the clamp is active, d angle_deg / d da = 180 / (pi * wa).
__device__ __forceinline__ void rot_delta_grad(const float* gb, const float* s, const float* box, const RotDecoded& k, const float* w, float* g) {
  g[0] = gb[0] * s[2] / w[0];
  g[1] = gb[1] * s[3] / w[1];
  g[2] = k.cw ? 0.f : gb[2] * box[2] / w[2];
  g[3] = k.ch ? 0.f : gb[3] * box[3] / w[3];
  g[4] = gb[4] * 180.f / (SOD_PI * w[4]);
}

// The IoU is iou_rotated_lds (the number NMS, the matcher and the evaluator see); a positive whose IoU is 0 has no gradient.
// HULL: with the hull term of rgiou_pair, which leaves such a positive a gradient.
template <bool HULL>
struct RotIouLoss {
  static constexpr int D = 5;
  static constexpr bool ROT_LDS = true;
  using Args = DecodeLossArgs;
  template <bool BWD>
  static __device__ __forceinline__ void positive(const Args& a, const float* p, long long r, long long i, P2* pts, float& acc, float* g) {
    float d[5], s[5], t[5], box[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) { d[e] = p[e]; s[e] = a.anchors[r * 5 + e]; t[e] = a.target[i * 5 + e]; }
    const RotDecoded k = rot_apply_deltas(d, s, a.w.w, a.clampv, box);
    const float iou = iou_rotated_lds(box, t, pts, 256);
    float gb[5];
    if constexpr (HULL) acc += rgiou_pair<BWD>(box, t, iou, gb);
    else acc += 1.f - iou;
    if (BWD && (HULL || iou > 0.f)) {
      if constexpr (!HULL) riou_grad(box, t, iou, gb);
      rot_delta_grad(gb, s, box, k, a.w.w, g);
    }
  }
};
using RiouLoss = RotIouLoss<false>;
using RgiouLoss = RotIouLoss<true>;

// The same decode, then the Gaussian KL-divergence loss of gauss_box_loss.h against the matched gt box: no clipping, so no LDS of its own.
struct RkldLoss {
  static constexpr int D = 5;
  static constexpr bool ROT_LDS = false;
  using Args = DecodeLossArgs;
  template <bool BWD>
  static __device__ __forceinline__ void positive(const Args& a, const float* p, long long r, long long i, P2* pts, float& acc, float* g) {
    float d[5], s[5], t[5], box[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) { d[e] = p[e]; s[e] = a.anchors[r * 5 + e]; t[e] = a.target[i * 5 + e]; }
    const RotDecoded k = rot_apply_deltas(d, s, a.w.w, a.clampv, box);
    float gb[5];
    acc += rkld_pair<BWD>(box, t, gb);
    if (BWD) rot_delta_grad(gb, s, box, k, a.w.w, g);
  }
};
