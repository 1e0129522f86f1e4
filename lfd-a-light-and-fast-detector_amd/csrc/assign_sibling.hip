// csrc/assign_sibling.hip -- training targets of the sibling meta-architectures, whole batch in one launch, one thread per
// (image, point), the image's boxes staged through LDS in chunks of kChunk (any G, G = 0 included).  Same conventions as
// lfd_assign_targets_f32 (targets.hip): points generated on the fly (level-major, row-major, x = j*stride, y = i*stride),
// fp32 in the reference's expression order (-ffp-contract=off, IEEE divide / sqrt).
//
//   * lfd_assign_targets_fcos_f32: FCOS.annotation_to_target (reference lfd/model/fcos.py:108-209; FCOSv1 :550-656 with
//     `multi_label`).  The reference builds [P, G] broadcasts, replaces the area of every invalid pair by INF = 1e8 and
//     takes `areas.min(dim=1)`; per point that is one pass over the boxes:
//       a[g]   = w*h if (min(dist) > 0 and lo <= max(dist) <= hi) else 1e8                     (fcos.py:159-173)
//       best   = first g with the smallest a[g]  (ties -> lowest box index; no valid box -> box 0)  (:175)
//       label  = gt_labels[best] if a[best] != 1e8 else num_classes                            (:178-181)
//       reg    = dist[best]                                                                     (:184)
//     multi_label (FCOSv1): labels[p, c] = 0 for every class c with a valid box at p, else 1    (:611-616)
//   * lfd_assign_targets_v2_f32: LFDv2._generate_target_for_single_image (reference lfd/model/lfdv2.py:278-418).
//     The reference sorts every row of the [P, G] scores ascending (stable), scatters the positive ones (the largest of a
//     class is written last) and takes the first maximum of the sorted row for the regression target; per point:
//       cls[p, c] = max score of the boxes of class c with score > 0, else 0                    (:395-405)
//       reg[p]    = delta of the box with the largest score; ties -- the all-zero row included -- go to the lowest box
//                   index (first maximum of a stably sorted ascending row)                      (:414-416)
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 64;
constexpr float kInf = 1e8f;   // fcos.py:9

struct Pt {
  float x, y;
  int level;
};

// level / coordinates of point p (generate_point_coordinates: x = j*stride, y = i*stride)
__device__ __forceinline__ Pt point_of(const int32_t* level_h, const int32_t* level_w, const int32_t* stride, int num_levels,
                                       int p) {
  int l = 0, q = p;
  while (l < num_levels - 1 && q >= level_h[l] * level_w[l]) { q -= level_h[l] * level_w[l]; ++l; }
  const int w = level_w[l] > 0 ? level_w[l] : 1;
  Pt r;
  r.x = (float)((q % w) * stride[l]);
  r.y = (float)((q / w) * stride[l]);
  r.level = l;
  return r;
}

struct GtArgs {
  const float* boxes;      // [num_boxes, 4] x, y, w, h
  const int64_t* labels;   // [num_boxes]
  const int32_t* offsets;  // [n + 1]
  int64_t num_boxes;
};

// rows [g0, g1) of image n, clamped to the buffer: a corrupt offsets array reads nothing out of bounds
__device__ __forceinline__ void image_rows(const GtArgs& g, int n, int64_t* g0, int64_t* g1) {
  int64_t a = g.offsets[n], b = g.offsets[n + 1];
  if (a < 0) a = 0;
  if (b > g.num_boxes) b = g.num_boxes;
  if (b < a) b = a;
  *g0 = a;
  *g1 = b;
}

__device__ __forceinline__ void stage_chunk(const GtArgs& g, int64_t base, int cnt, float* s_box, int* s_lab) {
  __syncthreads();
  for (int i = threadIdx.x; i < cnt * 4; i += blockDim.x) s_box[i] = g.boxes[base * 4 + i];
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) s_lab[i] = (int)g.labels[base + i];
  __syncthreads();
}

struct FcosArgs {
  lfd_assign_fcos_desc_t d;
  GtArgs gt;
  int64_t* labels;   // [n, P] | [n, P, C]
  float* reg_t;      // [n, P, 4]
};

__global__ __launch_bounds__(kThreads) void k_assign_fcos(FcosArgs a) {
  __shared__ float s_box[kChunk * 4];
  __shared__ int s_lab[kChunk];
  const int P = a.d.total_points, C = a.d.num_classes;
  const int n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid_pt = p < P;
  int64_t g0, g1;
  image_rows(a.gt, n, &g0, &g1);
  Pt pt = {0.f, 0.f, 0};
  if (valid_pt) pt = point_of(a.d.level_h, a.d.level_w, a.d.stride, a.d.num_levels, p);
  const float lo = a.d.range_lo[pt.level], hi = a.d.range_hi[pt.level];
  int64_t* mrow = a.labels + ((size_t)n * P + p) * C;
  if (valid_pt && a.d.multi_label)
    for (int c = 0; c < C; ++c) mrow[c] = 1;

  float best_a = 0.f;
  int best_lab = 0;
  bool have = false;
  float bd[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t base = g0; base < g1; base += kChunk) {
    const int cnt = (g1 - base) < kChunk ? (int)(g1 - base) : kChunk;
    stage_chunk(a.gt, base, cnt, s_box, s_lab);
    if (!valid_pt) continue;
    for (int g = 0; g < cnt; ++g) {
      const float bx = s_box[4 * g], by = s_box[4 * g + 1], bw = s_box[4 * g + 2], bh = s_box[4 * g + 3];
      const float d0 = pt.x - bx, d1 = pt.y - by;                                   // fcos.py:146-149
      const float d2 = (bx + bw - 1.f) - pt.x, d3 = (by + bh - 1.f) - pt.y;
      const float mn = fminf(fminf(d0, d1), fminf(d2, d3)), mx = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3));
      const bool ok = (mn > 0.f) && (mx >= lo) && (mx <= hi);                       // :159-164
      const float area = ok ? bw * bh : kInf;                                       // :173
      const int c = s_lab[g];
      if (ok && a.d.multi_label && c >= 0 && c < C) mrow[c] = 0;
      if (!have || area < best_a) {                                                 // first minimum
        have = true;
        best_a = area;
        best_lab = c;
        bd[0] = d0; bd[1] = d1; bd[2] = d2; bd[3] = d3;
      }
    }
  }
  if (!valid_pt) return;
  if (!a.d.multi_label) a.labels[(size_t)n * P + p] = (have && best_a != kInf) ? (int64_t)best_lab : (int64_t)C;
  *reinterpret_cast<float4*>(a.reg_t + ((size_t)n * P + p) * 4) = make_float4(bd[0], bd[1], bd[2], bd[3]);
}

struct V2Args {
  lfd_assign_desc_t d;
  GtArgs gt;
  float* cls_t;   // [n, P, C]
  float* reg_t;   // [n, P, 4]
};

__global__ __launch_bounds__(kThreads) void k_assign_v2(V2Args a) {
  __shared__ float s_box[kChunk * 4];
  __shared__ int s_lab[kChunk];
  const int P = a.d.total_points, C = a.d.num_classes;
  const int n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid_pt = p < P;
  int64_t g0, g1;
  image_rows(a.gt, n, &g0, &g1);
  Pt pt = {0.f, 0.f, 0};
  if (valid_pt) pt = point_of(a.d.level_h, a.d.level_w, a.d.stride, a.d.num_levels, p);
  const int l = pt.level;
  const float half = (float)a.d.stride[l] / 2.f;                                    // lfdv2.py:340
  const float rlo = (float)a.d.reg_lo[l], rhi = (float)a.d.reg_hi[l], glo = (float)a.d.gray_lo[l], ghi = (float)a.d.gray_hi[l];
  const float left_den = fmaxf((float)(a.d.reg_lo[l] - a.d.gray_lo[l]), 0.01f);     // :368
  const float right_den = fmaxf((float)(a.d.gray_hi[l] - a.d.reg_hi[l]), 0.01f);    // :373
  float* crow = a.cls_t + ((size_t)n * P + p) * C;
  if (valid_pt)
    for (int c = 0; c < C; ++c) crow[c] = 0.f;

  float best_s = 0.f;
  bool have = false;
  float bd[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t base = g0; base < g1; base += kChunk) {
    const int cnt = (g1 - base) < kChunk ? (int)(g1 - base) : kChunk;
    stage_chunk(a.gt, base, cnt, s_box, s_lab);
    if (!valid_pt) continue;
    for (int g = 0; g < cnt; ++g) {
      const float bx = s_box[4 * g], by = s_box[4 * g + 1], bw = s_box[4 * g + 2], bh = s_box[4 * g + 3];
      const float cx = bx + bw / 2.f, cy = by + bh / 2.f;                           // :306-307
      float d0 = pt.x - bx, d1 = pt.y - by;                                         // :312-315
      float d2 = (bx + bw - 1.f) - pt.x, d3 = (by + bh - 1.f) - pt.y;
      const bool hit = fminf(fminf(d0, d1), fminf(d2, d3)) >= 0.f;                  // :317
      // centerness-like score (:331-337): the deltas of a missed box are multiplied by 0, its score is 0
      float score = 0.f;
      if (hit) {
        const float lr = fmaxf(fminf(d0, d2), 0.f) / fmaxf(fmaxf(d0, d2), 0.01f);
        const float tb = fmaxf(fminf(d1, d3), 0.f) / fmaxf(fmaxf(d1, d3), 0.01f);
        score = sqrtf(lr * tb);
      }
      const bool core = (pt.x >= cx - half) && (pt.x <= cx + half) && (pt.y >= cy - half) && (pt.y <= cy + half) && hit;   // :340-347
      score = score * (core ? 0.f : 1.f) + (core ? 1.f : 0.f);                      // :348
      float measure;
      switch (a.d.assign_mode) {                                                    // :352-359
        case 0: measure = fmaxf(bw, bh); break;
        case 1: measure = fminf(bw, bh); break;
        case 2: measure = sqrtf(bw * bh); break;
        default: measure = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)); break;
      }
      if (a.d.independent) { d0 = d0 / rhi; d1 = d1 / rhi; d2 = d2 / rhi; d3 = d3 / rhi; }   // :363-364
      // relaxation across the gray band (:368-378): left * left_on + inside + right * right_on
      const float left = (measure - glo) / left_den;
      const float left_on = ((glo <= measure) && (measure < rlo)) ? 1.f : 0.f;
      const float inside = ((rlo <= measure) && (measure <= rhi)) ? 1.f : 0.f;
      const float right = (ghi - measure) / right_den;
      const float right_on = ((rhi < measure) && (measure <= ghi)) ? 1.f : 0.f;
      score = score * (left * left_on + inside + right * right_on);
      const int c = s_lab[g];
      if (score > 0.f && c >= 0 && c < C && score > crow[c]) crow[c] = score;       // :380,395-405
      if (!have || score > best_s) {                                                // first maximum (:414)
        have = true;
        best_s = score;
        bd[0] = d0; bd[1] = d1; bd[2] = d2; bd[3] = d3;
      }
    }
  }
  if (valid_pt) *reinterpret_cast<float4*>(a.reg_t + ((size_t)n * P + p) * 4) = make_float4(bd[0], bd[1], bd[2], bd[3]);
}

int check_levels(int n, int num_levels, const int32_t* level_h, const int32_t* level_w, const int32_t* stride, int total_points,
                 int num_classes) {
  if (n < 1 || num_levels < 1 || num_levels > LFD_MAX_LEVELS || num_classes < 1 || total_points < 0)
    return LFD_ERR_INVALID_ARGUMENT;
  long long pts = 0;
  for (int i = 0; i < num_levels; ++i) {
    if (level_h[i] < 0 || level_w[i] < 0 || stride[i] < 1) return LFD_ERR_INVALID_ARGUMENT;
    pts += (long long)level_h[i] * level_w[i];
  }
  if (pts != total_points) return LFD_ERR_INVALID_ARGUMENT;
  return LFD_OK;
}

// gt_offsets lives on the device; the caller's host copy (nullable) is what can be checked before the launch
int check_gt(int n, const float* gt_boxes, const int64_t* gt_labels, int64_t num_boxes, const int32_t* gt_offsets,
             const int32_t* gt_offsets_host) {
  if (!gt_offsets || num_boxes < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (num_boxes > 0 && (!gt_boxes || !gt_labels)) return LFD_ERR_INVALID_ARGUMENT;
  if (gt_offsets_host) {
    if (gt_offsets_host[0] < 0 || gt_offsets_host[n] > num_boxes) return LFD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
      if (gt_offsets_host[i + 1] < gt_offsets_host[i]) return LFD_ERR_INVALID_ARGUMENT;
  }
  return LFD_OK;
}

}  // namespace

extern "C" {

int lfd_assign_targets_fcos_f32(const lfd_assign_fcos_desc_t* d, const float* gt_boxes, const int64_t* gt_labels,
                                int64_t num_boxes, const int32_t* gt_offsets, const int32_t* gt_offsets_host,
                                int64_t* labels, float* reg_targets, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!d || !labels || !reg_targets) return LFD_ERR_INVALID_ARGUMENT;
  int rc = check_levels(d->n, d->num_levels, d->level_h, d->level_w, d->stride, d->total_points, d->num_classes);
  if (rc != LFD_OK) return rc;
  for (int i = 0; i < d->num_levels; ++i)
    if (!(d->range_lo[i] <= d->range_hi[i])) return LFD_ERR_INVALID_ARGUMENT;
  rc = check_gt(d->n, gt_boxes, gt_labels, num_boxes, gt_offsets, gt_offsets_host);
  if (rc != LFD_OK) return rc;
  if (d->total_points == 0) return LFD_OK;
  FcosArgs a{*d, {gt_boxes, gt_labels, gt_offsets, num_boxes}, labels, reg_targets};
  hipLaunchKernelGGL(k_assign_fcos, dim3((d->total_points + kThreads - 1) / kThreads, d->n), dim3(kThreads), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_assign_targets_v2_f32(const lfd_assign_desc_t* d, const float* gt_boxes, const int64_t* gt_labels, int64_t num_boxes,
                              const int32_t* gt_offsets, const int32_t* gt_offsets_host, float* cls_targets,
                              float* reg_targets, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!d || !cls_targets || !reg_targets) return LFD_ERR_INVALID_ARGUMENT;
  int rc = check_levels(d->n, d->num_levels, d->level_h, d->level_w, d->stride, d->total_points, d->num_classes);
  if (rc != LFD_OK) return rc;
  if (d->assign_mode < 0 || d->assign_mode > 3) return LFD_ERR_INVALID_ARGUMENT;
  rc = check_gt(d->n, gt_boxes, gt_labels, num_boxes, gt_offsets, gt_offsets_host);
  if (rc != LFD_OK) return rc;
  if (d->total_points == 0) return LFD_OK;
  V2Args a{*d, {gt_boxes, gt_labels, gt_offsets, num_boxes}, cls_targets, reg_targets};
  hipLaunchKernelGGL(k_assign_v2, dim3((d->total_points + kThreads - 1) / kThreads, d->n), dim3(kThreads), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
