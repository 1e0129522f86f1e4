// csrc/getloss_fcos.hip -- FCOS.get_loss / FCOSv1.get_loss (reference lfd/model/fcos.py:240-317, :687-768) as three
// launches with the shape of getloss.hip: no nonzero() gather, no per-module launches, no host sync.  Every (image, point)
// row contributes its sigmoid-focal term (all C logits against the row's label; in `multi_label` mode the C one-class
// terms of FCOSv1's flattened [N*P*C, 1] logits) and -- when it is positive (label != C; any class present for FCOSv1) --
//   ctr_t = sqrt(min(l,r)/max(l,r) * min(t,b)/max(t,b)) of its regression TARGET (fcos.py:211-215: a constant),
//   the IoU / GIoU / DIoU / CIoU loss of distance2bbox(point, prediction) against distance2bbox(point, target) times ctr_t
//   (fcos.py:297-303), and BCE-with-logits of the centerness logit against ctr_t (:304-305)
// to fp64 block partials; a fixed-order second stage makes the sums deterministic.  `finalize` applies the reference's
// normalisers -- num_pos + N for classification (:287), sum(ctr_t) for regression (:303), n_pos for centerness (mean) --
// on the GLOBAL sums of image-parallel ranks (same convention as lfd_get_loss_finalize_f32).  With no positive the
// regression and centerness losses are 0 with zero gradient (:306-308: sums over empty tensors).
// HBM-bound: one read of (C + 4 + 1) prediction floats, the labels and 4 target floats per row.
#include "common.h"
#include "loss_elems.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kSums = 8;   // cls_sum, weighted reg_sum, ctr_sum, n_pos, sum of centerness targets, (3 spare = 0)
constexpr int kUsed = 5;

struct Pt { float x, y; };

__device__ __forceinline__ Pt point_of(const lfd_fcos_loss_desc_t& d, int p) {
  int l = 0, base = 0;
  for (; l < d.num_levels - 1; ++l) {
    const int cnt = d.level_h[l] * d.level_w[l];
    if (p < base + cnt) break;
    base += cnt;
  }
  const int q = p - base, w = d.level_w[l];
  const int i = q / w, j = q - i * w;
  Pt r;
  r.x = (float)(j * d.stride[l]);   // generate_point_coordinates fcos.py:82-106 (no half-stride offset)
  r.y = (float)(i * d.stride[l]);
  return r;
}

__device__ __forceinline__ float4 box_of(Pt pt, float4 d) {   // distance2bbox fcos.py:217-238
  return make_float4(pt.x - d.x, pt.y - d.y, pt.x + d.z, pt.y + d.w);
}

__device__ __forceinline__ float centerness_of(float4 t) {   // fcos.py:211-215
  return sqrtf((fminf(t.x, t.z) / fmaxf(t.x, t.z)) * (fminf(t.y, t.w) / fmaxf(t.y, t.w)));
}

// positive row?  labels: [rows] (label != C) or, multi_label, [rows, C] with 0 = class present (fcos.py:284, :715-716)
__device__ __forceinline__ bool row_positive(const lfd_fcos_loss_desc_t& d, const int64_t* __restrict__ lab, int64_t row) {
  if (!d.multi_label) return lab[row] != d.num_classes;
  bool any = false;
  for (int c = 0; c < d.num_classes; ++c) any |= lab[row * d.num_classes + c] == 0;
  return any;
}

__device__ __forceinline__ float box_loss_value(const lfd_fcos_loss_desc_t& d, float4 pb, float4 tb) {
  return d.box_loss == 0 ? iou_loss_elem(pb, tb, d.box_eps) : box_loss(pb, tb, d.box_loss, d.box_eps).v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_fcos_partial(lfd_fcos_loss_desc_t d, const float* __restrict__ pc,
                                                          const float* __restrict__ pr, const float* __restrict__ pt_,
                                                          const int64_t* __restrict__ lab, const float* __restrict__ rt,
                                                          double* partials) {
  __shared__ double sm[kThreads / 64][kUsed];
  const int C = d.num_classes, P = d.total_points;
  const int64_t rows = (int64_t)d.n * P;
  double a_cls = 0.0, a_reg = 0.0, a_ctr = 0.0, a_w = 0.0;
  int a_pos = 0;
  for (int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x; row < rows; row += (int64_t)gridDim.x * kThreads) {
    const float* x = pc + row * C;
    float s = 0.f;
    if (d.multi_label) {
      for (int j = 0; j < C; ++j) s += focal_fwd_elem(x[j], (int)lab[row * C + j], 0, d.gamma, d.alpha);
    } else {
      const int label = (int)lab[row];
      for (int j = 0; j < C; ++j) s += focal_fwd_elem(x[j], label, j, d.gamma, d.alpha);
    }
    a_cls += (double)s;
    if (!row_positive(d, lab, row)) continue;
    ++a_pos;
    const Pt pt = point_of(d, (int)(row % P));
    const float4 r = *reinterpret_cast<const float4*>(pr + row * 4);
    const float4 t = *reinterpret_cast<const float4*>(rt + row * 4);
    const float ct = centerness_of(t);
    a_w += (double)ct;
    a_reg += (double)(box_loss_value(d, box_of(pt, r), box_of(pt, t)) * ct);
    a_ctr += (double)bce_logits(pt_[row], ct);
  }
  double v[kUsed] = {a_cls, a_reg, a_ctr, (double)a_pos, a_w};
#pragma unroll
  for (int k = 0; k < kUsed; ++k) v[k] = wave_sum_d(v[k]);
  if (lfd_lane() == 0)
    for (int k = 0; k < kUsed; ++k) sm[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < kUsed) {
    double s = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) s += sm[i][threadIdx.x];
    partials[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

// reduction of the block partials: wave k sums component k (lanes stride over the blocks, fixed butterfly)
__global__ __launch_bounds__(64 * kSums) void k_fcos_sums(const double* partials, int nblocks, double* sums) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  if (k < kUsed)
    for (int i = lane; i < nblocks; i += 64) s += partials[(size_t)i * kSums + k];
  s = wave_sum_d(s);
  if (lane == 0) sums[k] = s;
}

// out: [0] classification loss, [1] regression loss, [2] centerness loss, [3] their sum, [4] global n_pos,
//      [5] avg_factor cls (n_pos + N), [6] avg_factor reg (sum of centerness targets), [7] rank scale
__global__ void k_fcos_finalize(lfd_fcos_loss_desc_t d, const double* local, const double* global, float scale, float* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float n_pos = (float)global[3];
  const float avg_c = n_pos + (float)d.n * scale;     // fcos.py:287, N = the global batch (equal per-rank batches)
  const float avg_r = (float)global[4];               // :303
  const float lc = d.cls_loss_weight * ((float)local[0] / avg_c) * scale;
  const float lr = n_pos > 0.f ? d.reg_loss_weight * ((float)local[1] / avg_r) * scale : 0.f;    // :306-308
  const float lt = n_pos > 0.f ? d.ctr_loss_weight * ((float)local[2] / n_pos) * scale : 0.f;
  out[0] = lc;
  out[1] = lr;
  out[2] = lt;
  out[3] = lc + lr + lt;
  out[4] = n_pos;
  out[5] = avg_c;
  out[6] = avg_r;
  out[7] = scale;
}

__global__ __launch_bounds__(kThreads) void k_fcos_bwd(lfd_fcos_loss_desc_t d, const float* __restrict__ pc,
                                                      const float* __restrict__ pr, const float* __restrict__ pt_,
                                                      const int64_t* __restrict__ lab, const float* __restrict__ rt,
                                                      const float* __restrict__ fin, const float* __restrict__ gout,
                                                      float* __restrict__ gcls, float* __restrict__ greg,
                                                      float* __restrict__ gctr) {
  const int C = d.num_classes, P = d.total_points;
  const int64_t rows = (int64_t)d.n * P;
  // every partial loss also flows through the total (gout[3])
  const bool any_pos = fin[4] > 0.f;
  const float g_c = (gout[0] + gout[3]) * d.cls_loss_weight * fin[7] / fin[5];
  const float g_r = any_pos ? (gout[1] + gout[3]) * d.reg_loss_weight * fin[7] / fin[6] : 0.f;
  const float g_t = any_pos ? (gout[2] + gout[3]) * d.ctr_loss_weight * fin[7] / fin[4] : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x; row < rows; row += (int64_t)gridDim.x * kThreads) {
    const float* x = pc + row * C;
    float* gx = gcls + row * C;
    if (d.multi_label) {
      for (int j = 0; j < C; ++j) gx[j] = focal_bwd_elem(x[j], (int)lab[row * C + j], 0, d.gamma, d.alpha, g_c);
    } else {
      const int label = (int)lab[row];
      for (int j = 0; j < C; ++j) gx[j] = focal_bwd_elem(x[j], label, j, d.gamma, d.alpha, g_c);
    }
    float4 gr = make_float4(0.f, 0.f, 0.f, 0.f);
    float gt = 0.f;
    if (any_pos && row_positive(d, lab, row)) {
      const Pt pt = point_of(d, (int)(row % P));
      const float4 r = *reinterpret_cast<const float4*>(pr + row * 4);
      const float4 t = *reinterpret_cast<const float4*>(rt + row * 4);
      const float ct = centerness_of(t);
      const float4 pb = box_of(pt, r), tb = box_of(pt, t);
      const float g = g_r * ct;
      float4 gb;
      if (d.box_loss == 0) {
        gb = iou_loss_grad_elem(pb, tb, d.box_eps, g);
      } else {
        const Dual l = box_loss(pb, tb, d.box_loss, d.box_eps);
        gb = make_float4(l.d[0] * g, l.d[1] * g, l.d[2] * g, l.d[3] * g);
      }
      gr = make_float4(-gb.x, -gb.y, gb.z, gb.w);   // x1 = px - d0, y1 = py - d1, x2 = px + d2, y2 = py + d3
      gt = g_t * (1.f / (1.f + expf(-pt_[row])) - ct);
    }
    *reinterpret_cast<float4*>(greg + row * 4) = gr;
    gctr[row] = gt;
  }
}

inline unsigned grid_for(int64_t rows) {
  int64_t b = (rows + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}

int check_desc(const lfd_fcos_loss_desc_t* d) {
  if (!d) return LFD_ERR_INVALID_ARGUMENT;
  if (d->n < 0 || d->num_levels < 1 || d->num_levels > LFD_MAX_LEVELS || d->num_classes < 1 || d->total_points < 0)
    return LFD_ERR_INVALID_ARGUMENT;
  if (d->box_loss < 0 || d->box_loss > 3) return LFD_ERR_INVALID_ARGUMENT;
  long long pts = 0;
  for (int i = 0; i < d->num_levels; ++i) {
    if (d->level_h[i] < 0 || d->level_w[i] < 0 || d->stride[i] < 1) return LFD_ERR_INVALID_ARGUMENT;
    pts += (long long)d->level_h[i] * d->level_w[i];
  }
  if (pts != d->total_points) return LFD_ERR_INVALID_ARGUMENT;
  return LFD_OK;
}

}  // namespace

extern "C" {

size_t lfd_fcos_loss_workspace_bytes(void) { return sizeof(double) * kSums * kMaxBlocks; }

int lfd_fcos_loss_sums_f32(const lfd_fcos_loss_desc_t* d, const float* pred_cls, const float* pred_reg, const float* pred_ctr,
                           const int64_t* labels, const float* reg_targets, void* workspace, size_t workspace_bytes,
                           double* sums, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = check_desc(d);
  if (rc != LFD_OK) return rc;
  if (!sums) return LFD_ERR_INVALID_ARGUMENT;
  const int64_t rows = (int64_t)d->n * d->total_points;
  if (rows == 0) {
    if (hipMemsetAsync(sums, 0, sizeof(double) * kSums, st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
    return LFD_OK;
  }
  if (!pred_cls || !pred_reg || !pred_ctr || !labels || !reg_targets || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < lfd_fcos_loss_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  const unsigned g = grid_for(rows);
  hipLaunchKernelGGL(k_fcos_partial, dim3(g), dim3(kThreads), 0, st, *d, pred_cls, pred_reg, pred_ctr, labels, reg_targets,
                     (double*)workspace);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_fcos_sums, dim3(1), dim3(64 * kSums), 0, st, (const double*)workspace, (int)g, sums);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_fcos_loss_finalize_f32(const lfd_fcos_loss_desc_t* d, const double* local_sums, const double* global_sums,
                               float rank_scale, float* out, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = check_desc(d);
  if (rc != LFD_OK) return rc;
  if (!local_sums || !global_sums || !out) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_fcos_finalize, dim3(1), dim3(64), 0, st, *d, local_sums, global_sums, rank_scale, out);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_fcos_loss_bwd_f32(const lfd_fcos_loss_desc_t* d, const float* pred_cls, const float* pred_reg, const float* pred_ctr,
                          const int64_t* labels, const float* reg_targets, const float* finalized, const float* grad_out,
                          float* grad_cls, float* grad_reg, float* grad_ctr, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = check_desc(d);
  if (rc != LFD_OK) return rc;
  const int64_t rows = (int64_t)d->n * d->total_points;
  if (rows == 0) return LFD_OK;
  if (!pred_cls || !pred_reg || !pred_ctr || !labels || !reg_targets || !finalized || !grad_out || !grad_cls || !grad_reg ||
      !grad_ctr)
    return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_fcos_bwd, dim3(grid_for(rows)), dim3(kThreads), 0, st, *d, pred_cls, pred_reg, pred_ctr, labels,
                     reg_targets, finalized, grad_out, grad_cls, grad_reg, grad_ctr);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
