// Non-maximum suppression the reference reaches through detectron2 / torchvision
// (sources absent from the reference tree; semantics restated in SURVEY.md Appendix C.12, C.15):
//   nms                      torchvision.ops.nms via detectron2.layers.batched_nms (call sites fcosv2.py:241, rpd.py:781,
//                            proposal_utils.py:115, roi_heads/fast_rcnn.py:103)
// Latency-bound: 64 x 64 blocks of pairwise IoU bits, then one workgroup per image scans them in score order; no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------- NMS
__device__ __forceinline__ bool iou_gt(const float* a, const float* b, float thr) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (sa + sb - inter) > thr;
}

#include "rotated_iou.h"

// Cheap NECESSARY conditions for IoU(a, b) > thr between two rotated boxes (cx, cy, w, h, angle) - the NMS kernels run the polygon clipping
// only for pairs that pass:
//   * area ratio, any thr: inter <= min(area), union >= max(area)  =>  IoU <= min / max;
//   * for thr >= 0.5 only: IoU > thr >= 1/2 means the intersection S covers more than half of EACH box; a rectangle K is convex and centrally
//     symmetric, so a convex subset that misses its centre c lies in a half-plane through c and has at most half of K's area - hence
//     each box's centre lies in the other box (rot_vertices' frame: w axis (cos, -sin), h axis (sin, cos)).
// Both are applied with a 1e-3 slack, far above the rounding of the float IoU they guard, so no pair the full computation would flag
// is dropped (checked against the oracle's keep sets: tests/test_gpu_rcnn.py, tests/test_gpu_detection_ops.py).  (cs = cos / sin of the angles, precomputed per box.)
__device__ __forceinline__ bool rot_pair_may_exceed(const float* a, float ca, float sa, const float* b, float cb, float sb, float thr) {
  // Boxes thinner than a pixel are left to the full computation: detectron2's clipping works with ABSOLUTE tolerances (1e-14, 1e-6, 1e-8
  // on quantities of order 1e6) and returns values unrelated to the true overlap there - which the oracle reproduces and the product must too.
  if (fminf(fminf(a[2], a[3]), fminf(b[2], b[3])) < 1.0f) return true;
  const float a1 = a[2] * a[3], a2 = b[2] * b[3];
  if (fminf(a1, a2) < thr * 0.999f * fmaxf(a1, a2)) return false;
  if (thr >= 0.5f) {
    const float dx = b[0] - a[0], dy = b[1] - a[1];
    if (fabsf(dx * ca - dy * sa) > 0.5005f * a[2] + 1e-3f || fabsf(dx * sa + dy * ca) > 0.5005f * a[3] + 1e-3f) return false;   // centre of b in a
    if (fabsf(dx * cb - dy * sb) > 0.5005f * b[2] + 1e-3f || fabsf(dx * sb + dy * cb) > 0.5005f * b[3] + 1e-3f) return false;   // centre of a in b
  }
  return true;
}

// ---------------------------------------------------------------------------------------------- batched class-aware NMS
// detectron2.layers.batched_nms / batched_nms_rotated + keep[: max_keep] for B images of M candidate slots each, without a host round
// trip: empty slots carry score -inf, the per-image candidate counts stay on the device, and the scan stops after max_keep survivors.
// Class offsets: axis-aligned  boxes + class * (max coordinate of the image + 1)                       (torchvision batched_nms)
//                rotated       centres + class * (max - min + 1), max = max(max(cx, cy) + max(w, h) / 2), min = min(min(cx, cy) - max(w, h) / 2)
template <int BD>
__global__ __launch_bounds__(1024) void nms_class_shift_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                               const int* __restrict__ classes, int M, float* __restrict__ shifted,
                                                               int* __restrict__ nvalid) {
  __shared__ float redmx[16], redmn[16];
  __shared__ unsigned cntw[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* bx = boxes + (long long)b * M * BD;
  const float* sc = scores + (long long)b * M;
  float mx = -3.0e38f, mn = 3.0e38f;
  unsigned cnt = 0;
  for (int i = tid; i < M; i += 1024)
    if (sc[i] > -3.0e38f) {
      ++cnt;
      if (BD == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) mx = fmaxf(mx, bx[i * 4 + k]);
      } else {
        const float half = fmaxf(bx[i * 5 + 2], bx[i * 5 + 3]) / 2.f;
        mx = fmaxf(mx, fmaxf(bx[i * 5], bx[i * 5 + 1]) + half);
        mn = fminf(mn, fminf(bx[i * 5], bx[i * 5 + 1]) - half);
      }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); mn = fminf(mn, __shfl_xor(mn, o, 64)); cnt += __shfl_xor(cnt, o, 64); }
  if ((tid & 63) == 0) { redmx[tid >> 6] = mx; redmn[tid >> 6] = mn; cntw[tid >> 6] = cnt; }
  __syncthreads();
  mx = redmx[0]; mn = redmn[0]; cnt = cntw[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) { mx = fmaxf(mx, redmx[w]); mn = fminf(mn, redmn[w]); cnt += cntw[w]; }
  const float step = BD == 4 ? mx + 1.f : mx - mn + 1.f;
  for (int i = tid; i < M; i += 1024) {
    const float off = sc[i] > -3.0e38f ? (float)classes[(long long)b * M + i] * step : 0.f;
#pragma unroll
    for (int k = 0; k < BD; ++k) shifted[((long long)b * M + i) * BD + k] = bx[i * BD + k] + ((BD == 4 || k < 2) ? off : 0.f);
  }
  if (tid == 0) nvalid[b] = (int)cnt;
}

// mask[b][i][w] bit j = IoU(box order[i], box order[64 w + j]) > thr for j > i; grid (words, words, B); n read per image (nvalid == NULL: n = M)
template <int BD>   // BD = 4 axis-aligned XYXY, 5 rotated
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, const long long* __restrict__ order,
                                                      const int* __restrict__ nvalid, int M, float thr,
                                                      unsigned long long* __restrict__ mask, int words) {
  const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;   // only the upper triangle is ever read: half of the grid leaves before it loads anything
  const int n = nvalid ? min(nvalid[b], M) : M;
  if (rb * 64 >= n || cb * 64 >= n) return;
  boxes += (long long)b * M * BD; order += (long long)b * M; mask += (long long)b * M * words;
  __shared__ float cbox[64 * BD];
  __shared__ float crad[64];
  const int lane = threadIdx.x;
  const int cj = cb * 64 + lane;
  if (cj < n) {
    const long long o = order[cj];
#pragma unroll
    for (int e = 0; e < BD; ++e) cbox[lane * BD + e] = boxes[o * BD + e];
    if (BD == 5) crad[lane] = 0.5f * sqrtf(cbox[lane * BD + 2] * cbox[lane * BD + 2] + cbox[lane * BD + 3] * cbox[lane * BD + 3]);
  }
  __syncthreads();
  const int i = rb * 64 + lane;
  const int cnt = min(64, n - cb * 64);
  if constexpr (BD == 4) {
    if (i >= n) return;
    float a[BD];
    const long long oi = order[i];
#pragma unroll
    for (int e = 0; e < BD; ++e) a[e] = boxes[oi * BD + e];
    unsigned long long bits = 0;
    for (int j = (rb == cb) ? lane + 1 : 0; j < cnt; ++j)
      if (iou_gt(a, cbox + j * BD, thr)) bits |= 1ull << j;
    mask[(long long)i * words + cb] = bits;
  } else {
    // Rotated boxes: the polygon-clipping IoU costs hundreds of instructions and only the few pairs that pass the circle test need it.
    // Looping "for j: if (near) iou" makes the WAVE pay it for every column some lane is near (RPN proposals of one level overlap
    // heavily: nearly all 64 columns, 9.1 ms per step for 16 x 10 000 candidates).  Instead: circle test for all 64 x 64 pairs (no
    // divergence), the surviving pairs compacted through LDS and dealt out evenly over the lanes, results OR-ed into the rows' words.
    __shared__ float rbox[64 * BD];
    __shared__ P2 rot_pts[24 * 64];
    __shared__ float ccs[64 * 2];
    __shared__ unsigned short pairs[64 * 64];
    __shared__ unsigned long long rbits[64];
    __shared__ int total_pairs;
    float a[BD] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      const long long oi = order[i];
#pragma unroll
      for (int e = 0; e < BD; ++e) { a[e] = boxes[oi * BD + e]; rbox[lane * BD + e] = a[e]; }
    }
    rbits[lane] = 0ull;
    if (cj < n) {
      const float th = cbox[lane * BD + 4] * 0.01745329251994329577f;
      ccs[lane * 2] = cosf(th); ccs[lane * 2 + 1] = sinf(th);
    }
    __syncthreads();
    const float ra = 0.5f * sqrtf(a[2] * a[2] + a[3] * a[3]);
    const float tha = a[4] * 0.01745329251994329577f, ca = cosf(tha), sa = sinf(tha);
    unsigned long long near = 0ull;
    if (i < n)
      for (int j = (rb == cb) ? lane + 1 : 0; j < cnt; ++j) {
        const float dx = a[0] - cbox[j * BD], dy = a[1] - cbox[j * BD + 1], rs = ra + crad[j];
        if (dx * dx + dy * dy <= rs * rs * 1.0001f && rot_pair_may_exceed(a, ca, sa, cbox + j * BD, ccs[j * 2], ccs[j * 2 + 1], thr)) near |= 1ull << j;
      }
    // exclusive prefix sum of the per-row pair counts over the wave
    const int mine = __popcll(near);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) total_pairs = incl;
    int off = incl - mine;
    for (unsigned long long m = near; m; m &= m - 1ull) pairs[off++] = (unsigned short)((lane << 6) | __builtin_ctzll(m));
    __syncthreads();
    const int total = total_pairs;
    for (int t = lane; t < total; t += 64) {
      const int pr = pairs[t];
      const int r = pr >> 6, j = pr & 63;
      float ar[BD];
#pragma unroll
      for (int e = 0; e < BD; ++e) ar[e] = rbox[r * BD + e];
      if (iou_rotated_lds(ar, cbox + j * BD, rot_pts + lane, 64) > thr) atomicOr(&rbits[r], 1ull << j);
    }
    __syncthreads();
    if (i < n) mask[(long long)i * words + cb] = rbits[lane];
  }
}

// one workgroup per image, boxes visited in score order in chunks of 64: wave 0 resolves a chunk against the chunk's own 64x64 diagonal
// block of the suppression matrix with wave shuffles (no barrier per box), then thread w ORs the rows of the chunk's survivors
// into word w of the "removed" bitmap.  2 barriers per 64 boxes instead of 2 per box (10 000 candidates: 3.5 ms -> ~0.5 ms).
// The count is read from device memory (nvalid == NULL: n = M) and the scan stops at max_keep survivors.
__global__ __launch_bounds__(1024) void nms_scan_kernel(const unsigned long long* __restrict__ mask, const long long* __restrict__ order,
                                                        const int* __restrict__ nvalid, int M, int words, int max_keep,
                                                        long long* __restrict__ keep, int* __restrict__ nkeep) {
  __shared__ unsigned long long removed[1024];
  __shared__ unsigned long long chunk_keep;
  const int b = blockIdx.x, w = threadIdx.x;
  const int n = nvalid ? min(nvalid[b], M) : M;
  mask += (long long)b * M * words; order += (long long)b * M; keep += (long long)b * max_keep;
  const int nw = (n + 63) / 64;
  if (w < words) removed[w] = 0;
  __syncthreads();
  int kept = 0;
  for (int c = 0; c < nw && kept < max_keep; ++c) {
    const int cnt = min(64, n - c * 64);
    if (w < 64) {
      const long long i = (long long)c * 64 + w;
      const unsigned long long diag = (w < cnt) ? mask[i * words + c] : 0ull;
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
      unsigned long long rem = removed[c], kb = 0ull;
      for (int j = 0; j < cnt; ++j) {
        const unsigned long long dj = ((unsigned long long)__shfl(dhi, j, 64) << 32) | (unsigned long long)__shfl(dlo, j, 64);
        if (!((rem >> j) & 1ull)) { kb |= 1ull << j; rem |= dj; }
      }
      if (w == 0) chunk_keep = kb;
    }
    __syncthreads();
    const unsigned long long kb = chunk_keep;
    {   // all 1024 threads: word ww = w % words, row slice sl = w / words of `slices`; independent loads, merged with ds_or_b64
      const int slices = 1024 / words;          // words <= 1024
      const int ww = w % words, sl = w / words;
      if (sl < slices && ww > c && ww < nw) {
        unsigned long long acc = 0ull;
        for (int j = sl; j < cnt; j += slices)
          if ((kb >> j) & 1ull) acc |= mask[((long long)c * 64 + j) * words + ww];
        if (acc) atomicOr(&removed[ww], acc);
      }
    }
    if (w < 64 && ((kb >> w) & 1ull)) {
      const int pos = kept + __popcll(kb & ((1ull << w) - 1ull));
      if (pos < max_keep) keep[pos] = order[(long long)c * 64 + w];
    }
    kept += __popcll(kb);
    __syncthreads();
  }
  if (w == 0) nkeep[b] = kept < max_keep ? kept : max_keep;
}

// The per-image glue of find_top_rpn_proposals (detectron2 proposal_utils; reference copy slender_det/modeling/proposal_generator/
// proposal_utils.py:45-120) for the whole batch: drop non-finite entries, clip to the image, drop boxes not larger than min_size.
// Dropped slots get score -inf (= empty for the batched NMS); the number of non-finite entries is counted in *bad.
template <int BD>
__global__ __launch_bounds__(256) void rpn_clip_filter_kernel(float* __restrict__ boxes, float* __restrict__ scores, const float* __restrict__ image_hw,
                                                              int B, int M, float min_size, int* __restrict__ bad) {
  const long long total = (long long)B * M;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / M);
    float* q = boxes + i * BD;
    const float h = image_hw[2 * b], w = image_hw[2 * b + 1];
    bool fin = isfinite(scores[i]);
#pragma unroll
    for (int k = 0; k < BD; ++k) fin = fin && isfinite(q[k]);
    if (!fin) { atomicAdd(bad, 1); scores[i] = -__builtin_inff(); continue; }
    bool keep;
    if (BD == 4) {
      q[0] = fminf(fmaxf(q[0], 0.f), w); q[1] = fminf(fmaxf(q[1], 0.f), h);
      q[2] = fminf(fmaxf(q[2], 0.f), w); q[3] = fminf(fmaxf(q[3], 0.f), h);
      keep = (q[2] - q[0] > min_size) && (q[3] - q[1] > min_size);
    } else {
      float ang = fmodf(q[4] + 180.0f, 360.0f);          // RotatedBoxes.normalize_angles: (a + 180) % 360 - 180, Python modulo
      if (ang < 0.f) ang += 360.0f;
      q[4] = ang - 180.0f;
      if (fabsf(q[4]) <= 1.0f) {                          // RotatedBoxes.clip: only nearly horizontal boxes
        float x1 = q[0] - q[2] / 2.0f, y1 = q[1] - q[3] / 2.0f, x2 = q[0] + q[2] / 2.0f, y2 = q[1] + q[3] / 2.0f;
        x1 = fminf(fmaxf(x1, 0.f), w); y1 = fminf(fmaxf(y1, 0.f), h); x2 = fminf(fmaxf(x2, 0.f), w); y2 = fminf(fmaxf(y2, 0.f), h);
        q[0] = (x1 + x2) / 2.0f; q[1] = (y1 + y2) / 2.0f;
        q[2] = fminf(q[2], x2 - x1); q[3] = fminf(q[3], y2 - y1);
      }
      keep = (q[2] > min_size) && (q[3] > min_size);
    }
    if (!keep) scores[i] = -__builtin_inff();
  }
}

}  // namespace

extern "C" long long sod_nms_workspace_bytes(int n) {
  const long long words = (n + 63) / 64;
  return (long long)n * words * 8;
}

template <int BD>   // the batched kernels with B = 1, the count known on the host (no nvalid) and no cap on the survivors
static int nms_single(const float* boxes, const long long* order, int n, float iou_threshold, long long* keep, int* num_keep, void* mask_ws, void* stream) {
  if (n < 0 || !num_keep || (n > 0 && (!boxes || !order || !keep || !mask_ws))) return SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(num_keep, 0, sizeof(int), st);
  const int words = (n + 63) / 64;
  if (words > 1024) return SOD_ESIZE;   // 65536 boxes per call (detectron2 switches to per-class loops above 40 000)
  hipError_t e = hipMemsetAsync(mask_ws, 0, (size_t)n * words * 8, st);
  if (e != hipSuccess) return (int)e;
  SOD_LAUNCH(nms_mask_kernel<BD>, dim3(words, words, 1), dim3(64), 0, st, boxes, order, (const int*)nullptr, n, iou_threshold, (unsigned long long*)mask_ws, words);
  SOD_LAUNCH(nms_scan_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long*)mask_ws, order, (const int*)nullptr, n, words, n, keep, num_keep);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_nms(const float* boxes, const long long* order, int n, float iou_threshold, long long* keep, int* num_keep, void* mask_ws, void* stream) {
  return nms_single<4>(boxes, order, n, iou_threshold, keep, num_keep, mask_ws, stream);
}

extern "C" int sod_nms_rotated(const float* boxes, const long long* order, int n, float iou_threshold, long long* keep, int* num_keep, void* mask_ws, void* stream) {
  return nms_single<5>(boxes, order, n, iou_threshold, keep, num_keep, mask_ws, stream);
}

extern "C" long long sod_batched_nms_workspace_bytes(int B, int M, int box_dim) {
  const long long words = (M + 63) / 64;
  return (long long)B * M * words * 8 + (long long)B * M * box_dim * (long long)sizeof(float) + (long long)B * (long long)sizeof(int);
}

// shifted boxes + per-image candidate count (first half of batched NMS); the caller sorts the scores (any stable descending sort)
// and then calls sod_batched_nms_run with the order.  ws layout: [mask][shifted boxes][nvalid].
extern "C" int sod_batched_nms_prepare(const float* boxes, const float* scores, const int* classes, int B, int M, int box_dim, void* ws, void* stream) {
  if (!boxes || !scores || !classes || !ws || B <= 0 || M <= 0 || M > 65536 || (box_dim != 4 && box_dim != 5)) return SOD_EARG;
  const long long words = (M + 63) / 64;
  float* shifted = (float*)((char*)ws + (long long)B * M * words * 8);
  int* nvalid = (int*)(shifted + (long long)B * M * box_dim);
  if (box_dim == 4) SOD_LAUNCH(nms_class_shift_kernel<4>, dim3(B), dim3(1024), 0, (hipStream_t)stream, boxes, scores, classes, M, shifted, nvalid);
  else SOD_LAUNCH(nms_class_shift_kernel<5>, dim3(B), dim3(1024), 0, (hipStream_t)stream, boxes, scores, classes, M, shifted, nvalid);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_batched_nms_run(const long long* order, int B, int M, int box_dim, float iou_threshold, int max_keep, long long* keep,
                                   int* num_keep, void* ws, void* stream) {
  if (!order || !keep || !num_keep || !ws || B <= 0 || M <= 0 || M > 65536 || max_keep <= 0 || (box_dim != 4 && box_dim != 5)) return SOD_EARG;
  const int words = (M + 63) / 64;
  if (words > 1024) return SOD_ESIZE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* mask = (unsigned long long*)ws;
  const float* shifted = (const float*)((char*)ws + (long long)B * M * words * 8);
  const int* nvalid = (const int*)(shifted + (long long)B * M * box_dim);
  hipError_t e = hipMemsetAsync(mask, 0, (size_t)B * M * words * 8, st);
  if (e != hipSuccess) return (int)e;
  if (box_dim == 4) SOD_LAUNCH(nms_mask_kernel<4>, dim3(words, words, B), dim3(64), 0, st, shifted, order, nvalid, M, iou_threshold, mask, words);
  else SOD_LAUNCH(nms_mask_kernel<5>, dim3(words, words, B), dim3(64), 0, st, shifted, order, nvalid, M, iou_threshold, mask, words);
  SOD_LAUNCH(nms_scan_kernel, dim3(B), dim3(1024), 0, st, (const unsigned long long*)mask, order, nvalid, M, words, max_keep, keep, num_keep);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_rpn_clip_filter(float* boxes, float* scores, const float* image_hw, int B, int M, int box_dim, float min_size, int* bad_count,
                                   void* stream) {
  if (!boxes || !scores || !image_hw || !bad_count || B <= 0 || M <= 0 || (box_dim != 4 && box_dim != 5)) return SOD_EARG;
  const int g = (int)min(((long long)B * M + 255) / 256, 4096LL);
  if (box_dim == 4) SOD_LAUNCH(rpn_clip_filter_kernel<4>, dim3(g), dim3(256), 0, (hipStream_t)stream, boxes, scores, image_hw, B, M, min_size, bad_count);
  else SOD_LAUNCH(rpn_clip_filter_kernel<5>, dim3(g), dim3(256), 0, (hipStream_t)stream, boxes, scores, image_hw, B, M, min_size, bad_count);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
