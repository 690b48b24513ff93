// The three classification losses of dna_cls_loss / dna_cls_head_fwd (cls_head.hip) and of
// dna_pool_head_fwd (pool_head.hip): the label, tie and out-of-range rules live here once.
#pragma once
#include <math.h>

#include "common.h"

namespace dna {

// One element of the regression (MSE) or multi-label (BCE with logits) loss in arithmetic T: its
// term is added to acc, its dlogits (times inv_n) comes back. cls_loss below walks a row with it;
// the wide pooling head (pool_head.hip) spreads the B x C elements over a grid.
template <typename T>
__device__ __forceinline__ float cls_loss_elem(int problem, T v, T yc, T inv_nt, double& acc) {
  if (problem == DNA_CLS_REGRESSION) {
    const T d = v - yc;
    acc += (double)d * (double)d;
    return (float)((T)2 * d * inv_nt);
  }
  // BCE with logits: max(v, 0) - v y + log1p(exp(-|v|))
  const T e = exp(-fabs(v));
  acc += (double)(fmax(v, (T)0) - v * yc + log1p(e));
  const T sig = v >= (T)0 ? (T)1 / ((T)1 + e) : e / ((T)1 + e);
  return (float)((sig - yc) * inv_nt);
}

// For one workgroup of 1024 threads: loss, dlogits and (single-label) pred of logits [B, C], a
// thread per row (b = tid, tid + 1024, ...). T is the arithmetic type of a row. float: what the
// DNABERT-2 head computes. double: a batch of a few rows leaves dlogits of magnitude 1 / B whose
// column sums (dbias) cancel to far smaller values, so dlogits carries its one rounding to fp32
// and nothing else (the pooling heads; B x C elements: the cost is not measurable). The maximum
// and the argmax are float comparisons in both. Row losses are widened to double, added per
// thread in row order and then over the threads by a fixed tree.
//   single label: labels int64 [B]; a label outside [0, C) adds the row's log-sum-exp alone
//   regression (MSE) and multi label (BCE with logits): labels fp32 [B, C]
template <typename T>
__device__ __forceinline__ void cls_loss(const float* logits, const void* labels, int problem,
                                         int B, int C, float* loss, float* dlogits,
                                         int64_t* pred) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  const double inv_n = 1.0 / (problem == DNA_CLS_SINGLE_LABEL ? (double)B : (double)B * C);
  const T inv_nt = (T)inv_n;
  double acc = 0.0;
  for (int b = tid; b < B; b += 1024) {
    const float* lg = logits + (size_t)b * C;
    float* dl = dlogits + (size_t)b * C;
    if (problem == DNA_CLS_SINGLE_LABEL) {
      float m = lg[0];
      int arg = 0;
      for (int c = 1; c < C; ++c) {
        const float v = lg[c];
        if (v > m) { m = v; arg = c; }  // strict: a tie keeps the lowest index
      }
      T s = (T)0;
      for (int c = 0; c < C; ++c) s += exp((T)lg[c] - (T)m);
      const T lse = (T)m + log(s);
      const long y = (long)reinterpret_cast<const int64_t*>(labels)[b];
      const bool ok = y >= 0 && y < C;
      acc += (double)(lse - (ok ? (T)lg[y] : (T)0));
      for (int c = 0; c < C; ++c)
        dl[c] = (float)((exp((T)lg[c] - lse) - (c == y ? (T)1 : (T)0)) * inv_nt);
      if (pred) pred[b] = arg;
    } else {
      const float* y = reinterpret_cast<const float*>(labels) + (size_t)b * C;
      for (int c = 0; c < C; ++c) dl[c] = cls_loss_elem<T>(problem, lg[c], y[c], inv_nt, acc);
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(red[0] * inv_n);
}

}  // namespace dna
