// The Gaussian KL-divergence loss of ONE rotated box pair (Yang et al., "Learning High-Precision Bounding Box for Rotated Object Detection
// via Kullback-Leibler Divergence", NeurIPS 2021) and its gradient w.r.t. the first box, as device code: shared by the pair operator
// (the RkldPair policy of rotated_kld_loss.hip) and the RkldLoss policy of box_loss_policy.h (retina_box_loss.hip, rows_box_loss.hip).  The including file
// places this header inside its own anonymous namespace (after common.h), like rotated_iou.h.
//
// A box (cx, cy, w, h, angle_deg) - width axis ax = (cos t, -sin t), height axis ay = (sin t, cos t) - is the Gaussian with mean (cx, cy)
// and covariance S = R diag(w^2 / 4, h^2 / 4) R^T.  For the prediction p and the target t:
//     D = KL(N_p || N_t) = 1/2 (mp - mt)^T St^-1 (mp - mt) + 1/2 Tr(St^-1 Sp) + 1/2 ln(|St| / |Sp|) - 1
//     L = 1 - 1 / (1 + ln(1 + D))                      in [0, 1), 0 exactly when the Gaussians coincide
// In the target's frame, with d = angle_p - angle_t, u = (mp - mt) . ax_t, v = (mp - mt) . ay_t:
//     D = 2 (u / wt)^2 + 2 (v / ht)^2 + 1/2 [(wp cos d / wt)^2 + (hp sin d / wt)^2 + (wp sin d / ht)^2 + (hp cos d / ht)^2]
//         + ln(wt / wp) + ln(ht / hp) - 1
// Quotients are formed first and squared afterwards, and the logarithm is taken of each ratio by itself: no intermediate leaves the
// float32 range while a quotient of two sides stays below 1.8e19 (a 8000 x 1.5e-5 px sliver against a 7000 x 1 px box: D = 1.3e14).
// The value clamps D at 0 (rounding leaves -1e-7 for near-identical boxes); the gradient uses D as it is.
// No clipping, no sort, no LDS, no dynamically indexed array: everything runs in registers.
// A side of either box that is not positive or not finite gives NaN, value and gradient.  A square box is an isotropic Gaussian: its
// angle does not enter D and has gradient 0 - the loss cannot orient a square.
#pragma once

constexpr float RKLD_D2R = 0.01745329251994329577f;

// -> L; if BWD, g[0..5) = d L / d pred (angle: per degree)
template <bool BWD>
__device__ __forceinline__ float rkld_pair(const float* pred, const float* gt, float* g) {
  const float wp = pred[2], hp = pred[3], wt = gt[2], ht = gt[3];
  const bool ok = wp > 0.f && hp > 0.f && wt > 0.f && ht > 0.f && fmaxf(fmaxf(wp, hp), fmaxf(wt, ht)) < INFINITY;
  const float tt = gt[4] * RKLD_D2R, dl = (pred[4] - gt[4]) * RKLD_D2R;
  const float ct = cosf(tt), st = sinf(tt), cd = cosf(dl), sd = sinf(dl);
  const float dx = pred[0] - gt[0], dy = pred[1] - gt[1];
  const float qu = (dx * ct - dy * st) / wt, qv = (dx * st + dy * ct) / ht;
  const float a = wp / wt, b = hp / wt, c = wp / ht, e = hp / ht;
  const float ac = a * cd, bs = b * sd, cs = c * sd, ec = e * cd;
  const float tr = (ac * ac + bs * bs) + (cs * cs + ec * ec);
  const float D = 2.f * (qu * qu + qv * qv) + 0.5f * tr + (logf(wt / wp) + logf(ht / hp)) - 1.f;
  const float nan = __builtin_nanf("");
  if (BWD) {
    const float t1 = 1.f + log1pf(D);
    const float dLdD = 1.f / (t1 * t1 * (1.f + D));
    const float fu = 4.f * (qu / wt), fv = 4.f * (qv / ht);
    const float dcx = fu * ct + fv * st, dcy = fv * ct - fu * st;
    const float dwp = (ac * cd) / wt + (cs * sd) / ht - 1.f / wp;
    const float dhp = (bs * sd) / wt + (ec * cd) / ht - 1.f / hp;
    const float dth = sd * cd * ((b - a) * (b + a) - (e - c) * (e + c)) * RKLD_D2R;
    g[0] = ok ? dLdD * dcx : nan;
    g[1] = ok ? dLdD * dcy : nan;
    g[2] = ok ? dLdD * dwp : nan;
    g[3] = ok ? dLdD * dhp : nan;
    g[4] = ok ? dLdD * dth : nan;
  }
  return ok ? 1.f - 1.f / (1.f + log1pf(fmaxf(D, 0.f))) : nan;
}
