// csrc/loss_elems.h -- per-element device functions shared by the stand-alone loss kernels (losses.hip, boxloss.hip,
// targets.hip) and the fused get_loss kernels (getloss.hip, getloss_ex.hip, getloss_fcos.hip), so both paths produce the
// same values.
#pragma once
#include <float.h>
#include <math.h>
#include "common.h"

// one element of SigmoidFocalLossForward (sigmoid_focal_loss_cuda.cu:31-57), fp32 math
static __device__ __forceinline__ float focal_fwd_elem(float x, int t, int d, float gamma, float alpha) {
  const float c1 = (float)(t == d);
  const float c2 = (float)((t >= 0) & (t != d));
  const float zn = 1.0f - alpha, zp = alpha;
  const float p = 1.f / (1.f + expf(-x));
  const float term1 = powf(1.f - p, gamma) * logf(fmaxf(p, FLT_MIN));
  const float ge = (float)(x >= 0.f);
  const float term2 = powf(p, gamma) * (-1.f * x * ge - logf(1.f + expf(x - 2.f * x * ge)));
  float l = 0.f;
  l += -c1 * term1 * zp;
  l += -c2 * term2 * zn;
  return l;
}

// one element of SigmoidFocalLossBackward (sigmoid_focal_loss_cuda.cu:69-95)
static __device__ __forceinline__ float focal_bwd_elem(float x, int t, int d, float gamma, float alpha, float g) {
  const float c1 = (float)(t == d);
  const float c2 = (float)((t >= 0) & (t != d));
  const float zn = 1.0f - alpha, zp = alpha;
  const float p = 1.f / (1.f + expf(-x));
  const float term1 = powf(1.f - p, gamma) * (1.f - p - (p * gamma * logf(fmaxf(p, FLT_MIN))));
  const float ge = (float)(x >= 0.f);
  const float term2 =
      powf(p, gamma) * ((-1.f * x * ge - logf(1.f + expf(x - 2.f * x * ge))) * (1.f - p) * gamma - p);
  float r = 0.f;
  r += -c1 * term1 * zp;
  r += -c2 * term2 * zn;
  return r * g;
}


// aligned IoU loss of one box pair (iou_loss.py:67-79 overlaps, :98-102 union clamp, :121-123 -log(clamp))
static __device__ __forceinline__ float iou_loss_elem(float4 a, float4 b, float eps) {
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float ov = w * h;
  const float a1 = (a.z - a.x) * (a.w - a.y);
  const float a2 = (b.z - b.x) * (b.w - b.y);
  const float un = fmaxf(a1 + a2 - ov, 1e-6f);
  const float iou = fmaxf(ov / un, eps);
  return -logf(iou);
}

// d loss / d pred for one pair, following autograd through the same expression graph:
//   loss = -log(q), q = max(ov/un, eps); un = max(a1+a2-ov, 1e-6); ov = w*h with clamps at 0;
//   torch.max / torch.min route the gradient to the larger / smaller operand (ties: split evenly
//   in ATen; ties have measure zero for float boxes and are resolved towards `pred` here).
static __device__ __forceinline__ float4 iou_loss_grad_elem(float4 a, float4 b, float eps, float dl) {
  const float ltx = fmaxf(a.x, b.x), lty = fmaxf(a.y, b.y);
  const float rbx = fminf(a.z, b.z), rby = fminf(a.w, b.w);
  const float wr = rbx - ltx, hr = rby - lty;
  const float w = fmaxf(wr, 0.f), h = fmaxf(hr, 0.f);
  const float ov = w * h;
  const float pw = a.z - a.x, ph = a.w - a.y;
  const float a1 = pw * ph;
  const float a2 = (b.z - b.x) * (b.w - b.y);
  const float ur = a1 + a2 - ov;
  const float un = fmaxf(ur, 1e-6f);
  const float q = ov / un;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q > eps) {  // clamp(min=eps) passes gradient only above eps
    const float dq = -dl / q;
    const float dov_direct = dq / un;
    const float dun = (ur > 1e-6f) ? (-dq * ov / (un * un)) : 0.f;
    const float dov = dov_direct - dun;  // un depends on -ov
    const float da1 = dun;
    const float dw = (wr > 0.f) ? dov * h : 0.f;
    const float dh = (hr > 0.f) ? dov * w : 0.f;
    if (a.z <= b.z) g.z += dw;
    if (a.x >= b.x) g.x -= dw;
    if (a.w <= b.w) g.w += dh;
    if (a.y >= b.y) g.y -= dh;
    g.z += da1 * ph; g.x -= da1 * ph;
    g.w += da1 * pw; g.y -= da1 * pw;
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------------
// GIoU / DIoU / CIoU (boxloss.hip's stand-alone kernel and the fused FCOS get_loss, getloss_fcos.hip): the loss
// expression on dual numbers -- value + the four partial derivatives w.r.t. the predicted x1, y1, x2, y2.
// ---------------------------------------------------------------------------------------------------------
struct Dual {
  float v;
  float d[4];
};

static __device__ __forceinline__ Dual cst(float v) { return Dual{v, {0.f, 0.f, 0.f, 0.f}}; }
static __device__ __forceinline__ Dual var(float v, int i) {
  Dual r = cst(v);
  r.d[i] = 1.f;
  return r;
}
static __device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) {
  return Dual{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2], a.d[3] + b.d[3]}};
}
static __device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) {
  return Dual{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2], a.d[3] - b.d[3]}};
}
static __device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v * b.v;
  for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
static __device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) {
  Dual r;
  r.v = a.v / b.v;
  const float inv = 1.f / b.v;
  for (int i = 0; i < 4; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
static __device__ __forceinline__ Dual operator+(const Dual& a, float c) { Dual r = a; r.v += c; return r; }
static __device__ __forceinline__ Dual operator*(const Dual& a, float c) {
  return Dual{a.v * c, {a.d[0] * c, a.d[1] * c, a.d[2] * c, a.d[3] * c}};
}
static __device__ __forceinline__ Dual dmax(const Dual& a, const Dual& b) { return a.v >= b.v ? a : b; }
static __device__ __forceinline__ Dual dmin(const Dual& a, const Dual& b) { return a.v <= b.v ? a : b; }
static __device__ __forceinline__ Dual clamp0(const Dual& a) { return a.v > 0.f ? a : cst(0.f); }   // .clamp(min=0)
static __device__ __forceinline__ Dual datan(const Dual& a) {
  const float g = 1.f / (1.f + a.v * a.v);
  return Dual{atanf(a.v), {a.d[0] * g, a.d[1] * g, a.d[2] * g, a.d[3] * g}};
}

// kind: 1 GIoU (iou_loss.py:127-169), 2 DIoU (:172-223), 3 CIoU (:226-283)
static __device__ __forceinline__ Dual box_loss(float4 p, float4 t, int kind, float eps) {
  const Dual x1 = var(p.x, 0), y1 = var(p.y, 1), x2 = var(p.z, 2), y2 = var(p.w, 3);
  const Dual tx1 = cst(t.x), ty1 = cst(t.y), tx2 = cst(t.z), ty2 = cst(t.w);
  const Dual w = clamp0(dmin(x2, tx2) - dmax(x1, tx1)), h = clamp0(dmin(y2, ty2) - dmax(y1, ty1));
  const Dual overlap = w * h;
  const Dual ap = (x2 - x1) * (y2 - y1);
  const Dual ag = cst((t.z - t.x) * (t.w - t.y));
  const Dual uni = ap + ag - overlap + eps;
  const Dual iou = overlap / uni;
  const Dual ew = clamp0(dmax(x2, tx2) - dmin(x1, tx1)), eh = clamp0(dmax(y2, ty2) - dmin(y1, ty1));
  if (kind == 1) {
    const Dual earea = ew * eh + eps;
    const Dual giou = iou - (earea - uni) / earea;
    return cst(1.f) - giou;
  }
  const Dual c2 = ew * ew + eh * eh + eps;
  const Dual dx = (tx1 + tx2) - (x1 + x2), dy = (ty1 + ty2) - (y1 + y2);
  const Dual rho2 = (dx * dx) * 0.25f + (dy * dy) * 0.25f;
  if (kind == 2) return cst(1.f) - (iou - rho2 / c2);
  const Dual w1 = x2 - x1, h1 = (y2 - y1) + eps;
  const float w2 = t.z - t.x, h2 = (t.w - t.y) + eps;
  const float factor = 4.f / (float)(M_PI * M_PI);
  const Dual da = cst(atanf(w2 / h2)) - datan(w1 / h1);
  const Dual v = (da * da) * factor;
  const Dual ciou = iou - (rho2 / c2 + (v * v) / (cst(1.f) - iou + v));
  return cst(1.f) - ciou;
}

// B(x, t) = max(x, 0) - x t + log(1 + exp(-|x|))  (F.binary_cross_entropy_with_logits), dB/dx = sigmoid(x) - t
static __device__ __forceinline__ float bce_logits(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// one (row, class) element of Quality Focal Loss (gfocal_loss.py:11-52) against the quality target t (the score at the
// label's channel, 0 elsewhere): l = B(x, t) |t - s|^beta, s = sigmoid(x);
//   dl/dx = (s - t) |t - s|^beta - B beta |t - s|^(beta-1) sign(t - s) s (1 - s)   (t is a constant)
struct LossGrad {
  float l, g;
};
static __device__ __forceinline__ LossGrad qfl_elem(float xv, float t, float beta) {
  const float s = 1.f / (1.f + expf(-xv));
  const float u = t - s, m = fabsf(u);
  const float b = bce_logits(xv, t);
  const float mb = powf(m, beta);
  const float sg = u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f);
  LossGrad r;
  r.l = b * mb;
  r.g = (s - t) * mb - b * beta * powf(m, beta - 1.f) * sg * s * (1.f - s);
  return r;
}
static __device__ __forceinline__ float qfl_fwd_elem(float xv, float t, float beta) { return qfl_elem(xv, t, beta).l; }
static __device__ __forceinline__ float qfl_bwd_elem(float xv, float t, float beta) { return qfl_elem(xv, t, beta).g; }

// one element of LFD's "independent" regression losses on x = pred - target: kind 1 smooth-L1 (smooth_l1_loss.py:11-22:
// 0.5 d^2 / beta below beta, d - 0.5 beta above), 2 L1 (:25-30), 3 MSE (mse_loss.py:11-13), with d loss / d pred.
// |x| has derivative sign(x) with sign(0) = 0, like torch.abs.
static __device__ __forceinline__ LossGrad pointwise_loss_elem(float x, int kind, float beta) {
  const float d = fabsf(x);
  const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  LossGrad r;
  if (kind == 1) {
    if (d < beta) { r.l = 0.5f * d * d / beta; r.g = sg * (d / beta); }
    else { r.l = d - 0.5f * beta; r.g = sg; }
  } else if (kind == 2) {
    r.l = d; r.g = sg;
  } else {
    r.l = x * x; r.g = 2.f * x;
  }
  return r;
}
