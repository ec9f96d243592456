// Test-time augmentation, the merge step (detectron2 GeneralizedRCNNWithTTA._inverse_augmented_boxes + the candidate list that
// _merge_detections hands to fast_rcnn_inference_single_image; detectron2's source is absent, DESIGN.md section 12 restates it): the
// detections of every augmented run of an image are mapped back to the image's output resolution - un-flip, scale, clip - and packed
// into the padded per-image candidate layout of sod_batched_nms_* (score -inf = empty slot).  One launch for all runs of all images,
// one thread per output slot, no atomics, no host read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/slender_hip.h"
#include "common.h"

namespace {

constexpr int TTA_THREADS = 256;

// One entry per (image, slot-of-the-run-inside-its-image) pair, indexed b * A + a; cnt = 0 where no run was given for the pair.
struct TtaRun {
  int off, cnt;         // first row of the run in the concatenated detections, number of rows (<= D)
  int flip;
  float wa;             // width of the augmented image (the un-flip mirrors about it)
  float sx, sy;         // W / w_a, H / h_a, rounded once from double by the host
  float W, H;           // output size of the run's image
};

struct TtaArgs {
  const float* boxes;
  const float* scores;
  const int* classes;
  float* out_boxes;
  float* out_scores;
  int* out_classes;
  int D, total;         // total = B * A * D
  float score_thresh;
  TtaRun run[SOD_TTA_MAX_RUNS];
};

__global__ __launch_bounds__(TTA_THREADS) void tta_merge_kernel(const TtaArgs a) {
  const int i = blockIdx.x * TTA_THREADS + threadIdx.x;
  if (i >= a.total) return;
  const int r = i / a.D, d = i - r * a.D;            // r < B * A <= SOD_TTA_MAX_RUNS (checked by the host)
  const int off = a.run[r].off, cnt = a.run[r].cnt, flip = a.run[r].flip;
  const float wa = a.run[r].wa, sx = a.run[r].sx, sy = a.run[r].sy, W = a.run[r].W, H = a.run[r].H;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  float s = -__builtin_inff();
  int c = 0;
  if (d < cnt) {
    const int t = off + d;                             // off + cnt <= T (checked by the host)
    const float4 p = reinterpret_cast<const float4*>(a.boxes)[t];
    const float sc = a.scores[t];
    const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w) && isfinite(sc);
    if (fin && sc > a.score_thresh) {
      float x1 = p.x, x2 = p.z;
      if (flip) { x1 = wa - p.z; x2 = wa - p.x; }     // HFlipTransform.inverse: the box's corners swap roles
      q.x = fminf(fmaxf(x1 * sx, 0.f), W);
      q.y = fminf(fmaxf(p.y * sy, 0.f), H);
      q.z = fminf(fmaxf(x2 * sx, 0.f), W);
      q.w = fminf(fmaxf(p.w * sy, 0.f), H);
      s = sc;
      c = a.classes[t];
    }
  }
  reinterpret_cast<float4*>(a.out_boxes)[i] = q;
  a.out_scores[i] = s;
  a.out_classes[i] = c;
}

}  // namespace

extern "C" int sod_tta_merge_candidates(const float* boxes, const float* scores, const int* classes, int T, const int* det_off, int S,
                                        const int* run_image, const int* run_slot, const int* run_h, const int* run_w, const int* run_flip,
                                        const float* run_sx, const float* run_sy, const int* out_hw, int B, int A, int D, float score_thresh,
                                        float* out_boxes, float* out_scores, int* out_classes, void* stream) {
  if (T < 0 || S < 0 || B <= 0 || A <= 0 || D <= 0 || (long long)B * A > SOD_TTA_MAX_RUNS || S > B * A) return SOD_EARG;
  if (!out_boxes || !out_scores || !out_classes || !out_hw || !det_off) return SOD_EARG;
  if (S > 0 && (!run_image || !run_slot || !run_h || !run_w || !run_flip || !run_sx || !run_sy)) return SOD_EARG;
  if (T > 0 && (!boxes || !scores || !classes)) return SOD_EARG;
  if (((uintptr_t)boxes | (uintptr_t)out_boxes) & 15) return SOD_EALIGN;
  const long long total = (long long)B * A * D;
  if (total > 0x7fffffffLL / 16) return SOD_ESIZE;
  TtaArgs a;
  a.boxes = boxes; a.scores = scores; a.classes = classes;
  a.out_boxes = out_boxes; a.out_scores = out_scores; a.out_classes = out_classes;
  a.D = D; a.total = (int)total; a.score_thresh = score_thresh;
  for (int r = 0; r < SOD_TTA_MAX_RUNS; ++r) a.run[r] = TtaRun{0, 0, 0, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool seen[SOD_TTA_MAX_RUNS] = {};
  if (det_off[0] < 0) return SOD_EARG;
  for (int s = 0; s < S; ++s) {
    const int cnt = det_off[s + 1] - det_off[s];
    if (cnt < 0 || cnt > D || det_off[s + 1] > T) return SOD_EARG;        // more detections than slots / rows that were not given
    const int b = run_image[s], sl = run_slot[s];
    if (b < 0 || b >= B || sl < 0 || sl >= A || run_h[s] <= 0 || run_w[s] <= 0) return SOD_EARG;
    if (out_hw[2 * b] <= 0 || out_hw[2 * b + 1] <= 0 || seen[b * A + sl]) return SOD_EARG;
    seen[b * A + sl] = true;
    a.run[b * A + sl] = TtaRun{det_off[s], cnt, run_flip[s] ? 1 : 0, (float)run_w[s], run_sx[s], run_sy[s], (float)out_hw[2 * b + 1], (float)out_hw[2 * b]};
  }
  SOD_LAUNCH(tta_merge_kernel, dim3((unsigned)((total + TTA_THREADS - 1) / TTA_THREADS)), dim3(TTA_THREADS), 0, (hipStream_t)stream, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
