// csrc/boxloss.hip -- GIoU / DIoU / CIoU box-regression losses (reference lfd/model/losses/iou_loss.py:127-283, the
// other members of LFD's "union" regression-loss family next to IoULoss, lfd.py:64-66), forward AND gradient in one pass.
//
// The gradient is not hand-derived: the loss expression is evaluated on dual numbers (value + the four partial
// derivatives w.r.t. the predicted x1, y1, x2, y2), i.e. forward-mode differentiation inside the kernel.  max / min /
// clamp route the derivative like torch's autograd (to the selected operand; exact ties have measure zero for float
// boxes and go to the first operand), so the result is what `loss.sum().backward()` produces on the reference's
// expression graph, with one read of the boxes and no saved intermediates.  Elementwise, HBM-bound.
#include <math.h>
#include "common.h"
#include "loss_elems.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

__global__ __launch_bounds__(kThreads) void k_box_loss(const float4* __restrict__ pred, const float4* __restrict__ target,
                                                      int64_t n, int kind, float eps, float* __restrict__ loss,
                                                      float4* __restrict__ dpred) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const Dual l = box_loss(pred[i], target[i], kind, eps);
    loss[i] = l.v;
    if (dpred) dpred[i] = make_float4(l.d[0], l.d[1], l.d[2], l.d[3]);
  }
}

// Elementwise regression losses of LFD's "independent" family (lfd.py:61-66): smooth-L1 (smooth_l1_loss.py:11-22:
// 0.5 d^2 / beta below beta, d - 0.5 beta above), L1 (:25-30) and MSE (mse_loss.py:11-13), loss and d loss / d pred
// in one pass.  kind: 1 smooth-L1, 2 L1, 3 MSE (pointwise_loss_elem, loss_elems.h: shared with the fused get_loss).
__global__ __launch_bounds__(kThreads) void k_pointwise_loss(const float* __restrict__ pred,
                                                            const float* __restrict__ target, int64_t n, int kind,
                                                            float beta, float* __restrict__ loss,
                                                            float* __restrict__ dpred) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const LossGrad e = pointwise_loss_elem(pred[i] - target[i], kind, beta);
    loss[i] = e.l;
    if (dpred) dpred[i] = e.g;
  }
}

// ---------------------------------------------------------------------------------------------------------
// The two remaining classification losses LFD accepts (lfd.py:52-56): binary cross-entropy with logits against float
// targets (bce_with_logits_loss.py:28-44 -> F.binary_cross_entropy_with_logits, reduction 'none') and Quality Focal Loss
// (gfocal_loss.py:11-52).  B(x, t) = max(x, 0) - x t + log(1 + exp(-|x|)),  dB/dx = sigmoid(x) - t.
// QFL row n, class c:  t = score[n] if c == label[n] (a foreground label) else 0;  l = B(x, t) |t - s|^beta, s = sigmoid(x);
//   dl/dx = (s - t) |t - s|^beta - B beta |t - s|^(beta-1) sign(t - s) s (1 - s);  the row loss is the sum over classes.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_bce_logits(const float* __restrict__ x, const float* __restrict__ t, int64_t n,
                                                        float* __restrict__ loss, float* __restrict__ dx) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float xv = x[i], tv = t[i];
    loss[i] = bce_logits(xv, tv);
    if (dx) dx[i] = 1.f / (1.f + expf(-xv)) - tv;
  }
}

__global__ __launch_bounds__(kThreads) void k_qfl(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                 const float* __restrict__ score, int64_t rows, int c, float beta,
                                                 float* __restrict__ loss, float* __restrict__ dx) {
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kThreads) {
    const int64_t lab = label[r];
    const float sc = score[r];
    float sum = 0.f;
    for (int j = 0; j < c; ++j) {
      const float xv = x[r * c + j];
      const float t = (lab == j) ? sc : 0.f;            // labels outside [0, c) are background: no positive class
      const LossGrad e = qfl_elem(xv, t, beta);          // loss_elems.h: shared with the fused get_loss
      sum += e.l;
      if (dx) dx[r * c + j] = e.g;
    }
    loss[r] = sum;
  }
}

}  // namespace

extern "C" {

int lfd_bce_with_logits_f32(const float* logits, const float* targets, int64_t n, float* loss, float* d_logits,
                            lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (n == 0) return LFD_OK;
  if (!logits || !targets || !loss) return LFD_ERR_INVALID_ARGUMENT;
  int64_t b = (n + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  hipLaunchKernelGGL(k_bce_logits, dim3((unsigned)b), dim3(kThreads), 0, st, logits, targets, n, loss, d_logits);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_quality_focal_loss_f32(const float* logits, const int64_t* labels, const float* scores, int64_t rows,
                               int32_t channels, float beta, float* loss, float* d_logits, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rows < 0 || channels < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (rows == 0) return LFD_OK;
  if (!logits || !labels || !scores || !loss) return LFD_ERR_INVALID_ARGUMENT;
  int64_t b = (rows + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  hipLaunchKernelGGL(k_qfl, dim3((unsigned)b), dim3(kThreads), 0, st, logits, labels, scores, rows, channels, beta, loss,
                     d_logits);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_pointwise_loss_f32(const float* pred, const float* target, int64_t n, int32_t kind, float beta, float* loss,
                           float* d_loss_d_pred, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n < 0 || kind < 1 || kind > 3 || (kind == 1 && !(beta > 0.f))) return LFD_ERR_INVALID_ARGUMENT;
  if (n == 0) return LFD_OK;
  if (!pred || !target || !loss) return LFD_ERR_INVALID_ARGUMENT;
  int64_t b = (n + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  hipLaunchKernelGGL(k_pointwise_loss, dim3((unsigned)b), dim3(kThreads), 0, st, pred, target, n, kind, beta, loss,
                     d_loss_d_pred);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_box_loss_f32(const float* pred, const float* target, int64_t n, int32_t kind, float eps, float* loss,
                     float* d_loss_d_pred, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n < 0 || kind < 1 || kind > 3) return LFD_ERR_INVALID_ARGUMENT;
  if (n == 0) return LFD_OK;
  if (!pred || !target || !loss) return LFD_ERR_INVALID_ARGUMENT;
  int64_t b = (n + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  hipLaunchKernelGGL(k_box_loss, dim3((unsigned)b), dim3(kThreads), 0, st, (const float4*)pred, (const float4*)target, n,
                     kind, eps, loss, (float4*)d_loss_d_pred);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
