// Packed (variable-length) ALiBi attention for DNABERT-2, forward and backward, gfx950.
//
// The batch arrives unpadded: qkv is [T, 3*H*64] over the T real tokens of all sequences, in
// row-major (sequence, position) order, and cu_seqlens[n] .. cu_seqlens[n+1] are the rows of
// sequence n (the reference's bert_padding.unpad_input layout, bert_layers.py). A query attends to
// the keys of its own sequence only:
//   out_i = sum_j softmax_j(q_i . k_j * scale - slope_h * |pos_i - pos_j|) v_j
// pos is the token's column in the padded rectangle it came from (`positions`), so a batch with a
// [PAD] in the middle of a row keeps the reference's bias; without `positions` it is i - cu[n].
//
// Structure (attention is 1 - 8 % of a layer at these lengths; the gain of the packed path is the
// rows that no longer exist, so the kernels are plain):
//  * one wave per (sequence, head, 64-row tile); the grid is nseq * ceil(max_seqlen / 64) x heads
//    and the tiles past a sequence's end exit at once;
//  * bf16: v_mfma_f32_32x32x16_bf16 with the "swapped" products of csrc/attention.hip (the row a
//    lane owns is the MFMA column, so its softmax statistics live in the lane pair (l, l ^ 32)):
//      forward  S^T = K Q^T,  O^T += V^T P^T
//      dQ       S^T, dP^T = V dO^T,  dQ^T += K^T dS^T          (queries on lanes, writes delta)
//      dK/dV    S = Q K^T, dP = dO V^T,  dV^T += dO^T P,  dK^T += Q^T dS      (keys on lanes)
//    the swept operand (K/V, or Q/dO) is staged per 64-row tile in LDS, rows past the sequence's
//    end as zeros; transposed operands come from ds_read_b64_tr_b16;
//  * fp32: one thread per query / key, exact arithmetic (the 1e-3 parity mode).
// Ragged tiles: a key (query) outside the sequence gets probability exactly 0 by a select on its
// index -- no -inf arithmetic except exp2(-inf) = 0 and the first running maximum, which is
// finite after the first tile because every tile swept holds at least one key of the sequence.
// Rows outside the sequence are never stored, and every global row index is clamped into
// [0, total_rows) before it becomes an address, so a malformed cu_seqlens gives wrong numbers but
// no out-of-bounds access. No atomics: dQ comes from the query-tile kernel, dK and dV from the
// key-tile kernel, each row written once.
#include "common.h"

namespace dna {
namespace attn_varlen {

constexpr int D = 64;        // head dim
constexpr int TILE = 64;     // rows per wave, and rows per LDS tile
constexpr int LDW = D + 8;   // LDS row stride in bf16 (144 B: 16-B aligned, rows 4 banks apart)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

typedef __attribute__((ext_vector_type(4))) short s16x4;

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float pair_sum(float x) { return x + __shfl_xor(x, 32, 64); }
__device__ __forceinline__ float pair_max(float x) { return fmaxf(x, __shfl_xor(x, 32, 64)); }

// Row offset inside a 32-row MFMA block of accumulator register r (plus 4 * (lane >> 5))
__device__ __forceinline__ constexpr int aoff(int r) { return (r & 3) + 8 * (r >> 2); }

// Global row of position k of the sequence starting at row cu0, clamped into the buffer
__device__ __forceinline__ size_t grow(int cu0, int k, int total) {
  long long r = (long long)cu0 + k;
  r = r < 0 ? 0 : r;
  return (size_t)(r < total ? r : total - 1);
}

// A[m = 32 dt + (lane & 31)][k] = tile[row0 + 16 s + k'][m] for one 16-row k-step, k' in the
// order the accumulator of a 32x32 block holds its rows (so a bf16-rounded accumulator is the
// matching B operand as it stands): ds_read_b64_tr_b16 over 4 rows x 16 columns per 16 lanes.
__device__ __forceinline__ bf16x8 tr_operand(const bf16* tile, int row0, int dt, int lane) {
  const int g16 = lane >> 4, i16 = lane & 15;
  const int row = row0 + 4 * (g16 >> 1) + (i16 >> 2);
  const int col = 32 * dt + 16 * (g16 & 1) + 4 * (i16 & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(tile + row * LDW + col));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(tile + (row + 8) * LDW + col));
  const bf16x4 a = __builtin_bit_cast(bf16x4, lo), b = __builtin_bit_cast(bf16x4, hi);
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// Stage rows [t0, t0 + 64) of a sequence into two LDS tiles: 64 columns starting at col_a / col_b
// of a row-major [total, ld_a] / [total, ld_b] tensor (zeros past the sequence's end).
__device__ __forceinline__ void stage_pair(bf16* A, bf16* B, const bf16* __restrict__ src_a,
                                           size_t ld_a, const bf16* __restrict__ src_b,
                                           size_t ld_b, int cu0, int len, int t0, int total,
                                           int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int cc = lane + 64 * i, r = cc >> 3, ch = cc & 7;
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[j] = (bf16)0.f; b[j] = (bf16)0.f; }
    if (t0 + r < len) {
      const size_t g = grow(cu0, t0 + r, total);
      a = *reinterpret_cast<const bf16x8*>(src_a + g * ld_a + ch * 8);
      b = *reinterpret_cast<const bf16x8*>(src_b + g * ld_b + ch * 8);
    }
    *reinterpret_cast<bf16x8*>(A + r * LDW + ch * 8) = a;
    *reinterpret_cast<bf16x8*>(B + r * LDW + ch * 8) = b;
  }
}

__device__ __forceinline__ float position_of(const int* __restrict__ positions, size_t g, int k) {
  return positions ? (float)positions[g] : (float)k;
}

// What a wave knows about its tile
struct Tile {
  int cu0, len, t0, h;
};
__device__ __forceinline__ bool decode(const int* __restrict__ cu, int ntile, Tile& t) {
  const int n = blockIdx.x / ntile;
  t.t0 = (blockIdx.x % ntile) * TILE;
  t.h = blockIdx.y;
  t.cu0 = cu[n];
  t.len = cu[n + 1] - t.cu0;
  return t.t0 < t.len;
}

// ----------------------------------------------------------------------------- bf16 forward
__global__ __launch_bounds__(64) void fwd_bf16_kernel(
    const bf16* __restrict__ qkv, const int* __restrict__ cu, const int* __restrict__ positions,
    const float* __restrict__ slopes, int ntile, int total, int H, float c,
    bf16* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[TILE * LDW];
  __shared__ __attribute__((aligned(16))) bf16 Vs[TILE * LDW];
  __shared__ __attribute__((aligned(16))) float kpos[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, ql = lane & 31, hh = lane >> 5;
  const int len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope2 = slopes[h] * LOG2E;
  const int nqh = t.t0 + 32 < len ? 2 : 1;  // 32-query halves with a query in the sequence

  bf16x8 qf[2][4];
  float qpos[2], m[2], l[2];
  size_t qrow[2];
  bool qok[2];
  f32x16 o[2][2];
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    const int qi = t.t0 + 32 * qh + ql, qc = min(qi, len - 1);
    qok[qh] = qi < len;
    qrow[qh] = grow(t.cu0, qc, total);
    qpos[qh] = position_of(positions, qrow[qh], qc);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      qf[qh][s] = *reinterpret_cast<const bf16x8*>(qkv + qrow[qh] * ld + h * D + 16 * s + 8 * hh);
    m[qh] = -INFINITY;
    l[qh] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[qh][0][r] = 0.f; o[qh][1][r] = 0.f; }
  }

  for (int k0 = 0; k0 < len; k0 += TILE) {
    __syncthreads();
    stage_pair(Ks, Vs, qkv + (size_t)H * D + h * D, ld, qkv + (size_t)2 * H * D + h * D, ld, t.cu0,
               len, k0, total, lane);
    kpos[lane] = k0 + lane < len
                     ? position_of(positions, grow(t.cu0, k0 + lane, total), k0 + lane) : 0.f;
    __syncthreads();
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      if (qh >= nqh) break;
      f32x16 sa[2];
      float mx = -INFINITY;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[kh][r] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bf16x8 ak =
              *reinterpret_cast<const bf16x8*>(Ks + (kh * 32 + ql) * LDW + 16 * s + 8 * hh);
          sa[kh] = mfma(ak, qf[qh][s], sa[kh]);  // S^T[key][q]
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 kp = *reinterpret_cast<const f32x4*>(kpos + kh * 32 + 8 * g + 4 * hh);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = k0 + kh * 32 + 8 * g + 4 * hh + e;
            const float x = fmaf(sa[kh][4 * g + e], c, -slope2 * fabsf(qpos[qh] - kp[e]));
            sa[kh][4 * g + e] = key < len ? x : -INFINITY;
            mx = fmaxf(mx, sa[kh][4 * g + e]);
          }
        }
      }
      // key k0 is in the sequence, so mx and with it the new maximum are finite
      const float mn = fmaxf(m[qh], pair_max(mx));
      const float alpha = ex2(m[qh] - mn);
      m[qh] = mn;
      float psum = 0.f;
      bf16x8 pb[2][2];
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = ex2(sa[kh][r] - mn);
          psum += p;
          pb[kh][r >> 3][r & 7] = (bf16)p;
        }
      l[qh] = fmaf(l[qh], alpha, psum);
#pragma unroll
      for (int r = 0; r < 16; ++r) { o[qh][0][r] *= alpha; o[qh][1][r] *= alpha; }
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)  // O^T[d][q] += V^T[d][key] P^T[key][q]
            o[qh][dt] = mfma(tr_operand(Vs, kh * 32 + 16 * s, dt, lane), pb[kh][s], o[qh][dt]);
    }
  }
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    if (qh >= nqh) break;
    const float lt = pair_sum(l[qh]);
    if (!qok[qh]) continue;
    const float inv = 1.f / lt;
    bf16* row = out + qrow[qh] * ((size_t)H * D) + h * D;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (bf16)(o[qh][dt][4 * g + e] * inv);
        *reinterpret_cast<bf16x4*>(row + 32 * dt + 8 * g + 4 * hh) = v;
      }
    if (hh == 0) lse[(size_t)h * total + qrow[qh]] = (m[qh] + __log2f(lt)) * LN2;
  }
}

// ----------------------------------------------------------------------------- bf16 dQ (+ delta)
__global__ __launch_bounds__(64) void dq_bf16_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ out, const bf16* __restrict__ dout,
    const float* __restrict__ lse, float* __restrict__ delta, const int* __restrict__ cu,
    const int* __restrict__ positions, const float* __restrict__ slopes, int ntile, int total,
    int H, float c, float scale, bf16* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[TILE * LDW];
  __shared__ __attribute__((aligned(16))) bf16 Vs[TILE * LDW];
  __shared__ __attribute__((aligned(16))) float kpos[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, ql = lane & 31, hh = lane >> 5;
  const int len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope2 = slopes[h] * LOG2E;
  const int nqh = t.t0 + 32 < len ? 2 : 1;

  bf16x8 qf[2][4], df[2][4];
  float qpos[2], lse2[2], dl[2];
  size_t qrow[2];
  bool qok[2];
  f32x16 dq[2][2];
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    const int qi = t.t0 + 32 * qh + ql, qc = min(qi, len - 1);
    qok[qh] = qi < len;
    qrow[qh] = grow(t.cu0, qc, total);
    qpos[qh] = position_of(positions, qrow[qh], qc);
    const size_t orow = qrow[qh] * ((size_t)H * D) + h * D;
    float acc = 0.f;  // delta = rowsum(dO * O): this lane holds half the row, lane ^ 32 the rest
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[qh][s] = *reinterpret_cast<const bf16x8*>(qkv + qrow[qh] * ld + h * D + 16 * s + 8 * hh);
      df[qh][s] = *reinterpret_cast<const bf16x8*>(dout + orow + 16 * s + 8 * hh);
      const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(out + orow + 16 * s + 8 * hh);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf((float)df[qh][s][j], (float)o8[j], acc);
    }
    dl[qh] = pair_sum(acc);
    lse2[qh] = lse[(size_t)h * total + qrow[qh]] * LOG2E;
    if (qok[qh] && hh == 0) delta[(size_t)h * total + qrow[qh]] = dl[qh];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[qh][0][r] = 0.f; dq[qh][1][r] = 0.f; }
  }

  for (int k0 = 0; k0 < len; k0 += TILE) {
    __syncthreads();
    stage_pair(Ks, Vs, qkv + (size_t)H * D + h * D, ld, qkv + (size_t)2 * H * D + h * D, ld, t.cu0,
               len, k0, total, lane);
    kpos[lane] = k0 + lane < len
                     ? position_of(positions, grow(t.cu0, k0 + lane, total), k0 + lane) : 0.f;
    __syncthreads();
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      if (qh >= nqh) break;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        f32x16 sa, pa;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa[r] = 0.f; pa[r] = -dl[qh]; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int off = (kh * 32 + ql) * LDW + 16 * s + 8 * hh;
          sa = mfma(*reinterpret_cast<const bf16x8*>(Ks + off), qf[qh][s], sa);  // S^T[key][q]
          pa = mfma(*reinterpret_cast<const bf16x8*>(Vs + off), df[qh][s], pa);  // dP^T - delta
        }
        bf16x8 db[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 kp = *reinterpret_cast<const f32x4*>(kpos + kh * 32 + 8 * g + 4 * hh);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e, key = k0 + kh * 32 + 8 * g + 4 * hh + e;
            const float x = fmaf(sa[r], c, -slope2 * fabsf(qpos[qh] - kp[e])) - lse2[qh];
            const float p = key < len ? ex2(x) : 0.f;
            db[r >> 3][r & 7] = (bf16)(p * pa[r]);
          }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)  // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
            dq[qh][dt] = mfma(tr_operand(Ks, kh * 32 + 16 * s, dt, lane), db[s], dq[qh][dt]);
      }
    }
  }
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    if (qh >= nqh || !qok[qh]) continue;
    bf16* row = dqkv + qrow[qh] * ld + h * D;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (bf16)(dq[qh][dt][4 * g + e] * scale);
        *reinterpret_cast<bf16x4*>(row + 32 * dt + 8 * g + 4 * hh) = v;
      }
  }
}

// ----------------------------------------------------------------------------- bf16 dK / dV
__global__ __launch_bounds__(64) void dkdv_bf16_kernel(
    const bf16* __restrict__ qkv, const bf16* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ cu,
    const int* __restrict__ positions, const float* __restrict__ slopes, int ntile, int total,
    int H, float c, float scale, bf16* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) bf16 Qs[TILE * LDW];
  __shared__ __attribute__((aligned(16))) bf16 Os[TILE * LDW];  // dO
  __shared__ __attribute__((aligned(16))) float qpos[TILE], ql2[TILE], qdl[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, kl = lane & 31, hh = lane >> 5;
  const int len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope2 = slopes[h] * LOG2E;
  const int nkb = t.t0 + 32 < len ? 2 : 1;  // 32-key blocks with a key in the sequence

  bf16x8 kf[2][4], vf[2][4];
  float kpos[2];
  size_t krow[2];
  bool kok[2];
  f32x16 dk[2][2], dv[2][2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const int kj = t.t0 + 32 * kb + kl, kc = min(kj, len - 1);
    kok[kb] = kj < len;
    krow[kb] = grow(t.cu0, kc, total);
    kpos[kb] = position_of(positions, krow[kb], kc);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16* src = qkv + krow[kb] * ld + h * D + 16 * s + 8 * hh;
      kf[kb][s] = *reinterpret_cast<const bf16x8*>(src + (size_t)H * D);
      vf[kb][s] = *reinterpret_cast<const bf16x8*>(src + (size_t)2 * H * D);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk[kb][0][r] = 0.f; dk[kb][1][r] = 0.f; dv[kb][0][r] = 0.f; dv[kb][1][r] = 0.f;
    }
  }

  for (int q0 = 0; q0 < len; q0 += TILE) {
    __syncthreads();
    stage_pair(Qs, Os, qkv + h * D, ld, dout + h * D, (size_t)H * D, t.cu0, len, q0, total, lane);
    {
      const bool in = q0 + lane < len;
      const size_t g = grow(t.cu0, q0 + lane, total);
      qpos[lane] = in ? position_of(positions, g, q0 + lane) : 0.f;
      ql2[lane] = in ? lse[(size_t)h * total + g] * LOG2E : 0.f;
      qdl[lane] = in ? delta[(size_t)h * total + g] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (kb >= nkb) break;
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        f32x16 sa, pa;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa[r] = 0.f; pa[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int off = (qh * 32 + kl) * LDW + 16 * s + 8 * hh;
          sa = mfma(*reinterpret_cast<const bf16x8*>(Qs + off), kf[kb][s], sa);  // S[q][key]
          pa = mfma(*reinterpret_cast<const bf16x8*>(Os + off), vf[kb][s], pa);  // dP[q][key]
        }
        bf16x8 pb[2], sb[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int qo = qh * 32 + 8 * g + 4 * hh;
          const f32x4 qp = *reinterpret_cast<const f32x4*>(qpos + qo);
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(ql2 + qo);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(qdl + qo);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const float x = fmaf(sa[r], c, -slope2 * fabsf(qp[e] - kpos[kb])) - l4[e];
            const float p = q0 + qo + e < len ? ex2(x) : 0.f;
            pb[r >> 3][r & 7] = (bf16)p;
            sb[r >> 3][r & 7] = (bf16)(p * (pa[r] - d4[e]));
          }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
            dv[kb][dt] = mfma(tr_operand(Os, qh * 32 + 16 * s, dt, lane), pb[s], dv[kb][dt]);
            dk[kb][dt] = mfma(tr_operand(Qs, qh * 32 + 16 * s, dt, lane), sb[s], dk[kb][dt]);
          }
      }
    }
  }
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    if (kb >= nkb || !kok[kb]) continue;
    bf16* row = dqkv + krow[kb] * ld + h * D;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 vk, vv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vk[e] = (bf16)(dk[kb][dt][4 * g + e] * scale);
          vv[e] = (bf16)dv[kb][dt][4 * g + e];
        }
        *reinterpret_cast<bf16x4*>(row + (size_t)H * D + 32 * dt + 8 * g + 4 * hh) = vk;
        *reinterpret_cast<bf16x4*>(row + (size_t)2 * H * D + 32 * dt + 8 * g + 4 * hh) = vv;
      }
  }
}

// ----------------------------------------------------------------------------- fp32 path
// One thread per query (key), the swept rows staged 64 at a time in LDS; only the rows of the
// sequence are visited, so nothing is masked.
__device__ __forceinline__ void stage_f32(float (*A)[D + 1], float (*B)[D + 1],
                                          const float* __restrict__ src_a, size_t ld_a,
                                          const float* __restrict__ src_b, size_t ld_b, int cu0,
                                          int len, int t0, int total, int lane) {
  for (int idx = lane; idx < TILE * D; idx += 64) {
    const int r = idx / D, d = idx % D;
    const size_t g = grow(cu0, min(t0 + r, len - 1), total);
    A[r][d] = src_a[g * ld_a + d];
    B[r][d] = src_b[g * ld_b + d];
  }
}

__global__ __launch_bounds__(64) void fwd_f32_kernel(
    const float* __restrict__ qkv, const int* __restrict__ cu, const int* __restrict__ positions,
    const float* __restrict__ slopes, int ntile, int total, int H, float scale,
    float* __restrict__ out, float* __restrict__ lse) {
  __shared__ float Kt[TILE][D + 1], Vt[TILE][D + 1];
  __shared__ float kpos[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope = slopes[h];
  const int qi = t.t0 + lane, qc = min(qi, len - 1);
  const size_t qrow = grow(t.cu0, qc, total);
  const float qp = position_of(positions, qrow, qc);
  float q[D], o[D];
  for (int d = 0; d < D; ++d) { q[d] = qkv[qrow * ld + h * D + d]; o[d] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < len; k0 += TILE) {
    __syncthreads();
    stage_f32(Kt, Vt, qkv + (size_t)H * D + h * D, ld, qkv + (size_t)2 * H * D + h * D, ld, t.cu0,
              len, k0, total, lane);
    const int kc = min(k0 + lane, len - 1);
    kpos[lane] = position_of(positions, grow(t.cu0, kc, total), kc);
    __syncthreads();
    const int kn = min(TILE, len - k0);
    for (int r = 0; r < kn; ++r) {
      float sdot = 0.f;
      for (int d = 0; d < D; ++d) sdot = fmaf(q[d], Kt[r][d], sdot);
      const float x = sdot * scale - slope * fabsf(qp - kpos[r]);
      const float mn = fmaxf(m, x);  // finite from the first key on
      const float a = __expf(m - mn), p = __expf(x - mn);
      l = l * a + p;
      for (int d = 0; d < D; ++d) o[d] = fmaf(p, Vt[r][d], o[d] * a);
      m = mn;
    }
  }
  if (qi < len) {
    float* orow = out + qrow * ((size_t)H * D) + h * D;
    for (int d = 0; d < D; ++d) orow[d] = o[d] / l;
    lse[(size_t)h * total + qrow] = m + __logf(l);
  }
}

__global__ void delta_f32_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                 int total, int H, float* __restrict__ delta) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (row, head)
  if (idx >= (size_t)total * H) return;
  const size_t row = idx / H;
  const int h = (int)(idx % H);
  const float* o = out + row * ((size_t)H * D) + h * D;
  const float* g = dout + row * ((size_t)H * D) + h * D;
  float acc = 0.f;
#pragma unroll 8
  for (int d = 0; d < D; ++d) acc = fmaf(o[d], g[d], acc);
  delta[(size_t)h * total + row] = acc;
}

__global__ __launch_bounds__(64) void dq_f32_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ cu,
    const int* __restrict__ positions, const float* __restrict__ slopes, int ntile, int total,
    int H, float scale, float* __restrict__ dqkv) {
  __shared__ float Kt[TILE][D + 1], Vt[TILE][D + 1];
  __shared__ float kpos[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope = slopes[h];
  const int qi = t.t0 + lane, qc = min(qi, len - 1);
  const size_t qrow = grow(t.cu0, qc, total);
  const float qp = position_of(positions, qrow, qc);
  float q[D], g[D], dq[D];
  for (int d = 0; d < D; ++d) {
    q[d] = qkv[qrow * ld + h * D + d];
    g[d] = dout[qrow * ((size_t)H * D) + h * D + d];
    dq[d] = 0.f;
  }
  const float L = lse[(size_t)h * total + qrow], dl = delta[(size_t)h * total + qrow];
  for (int k0 = 0; k0 < len; k0 += TILE) {
    __syncthreads();
    stage_f32(Kt, Vt, qkv + (size_t)H * D + h * D, ld, qkv + (size_t)2 * H * D + h * D, ld, t.cu0,
              len, k0, total, lane);
    const int kc = min(k0 + lane, len - 1);
    kpos[lane] = position_of(positions, grow(t.cu0, kc, total), kc);
    __syncthreads();
    const int kn = min(TILE, len - k0);
    for (int r = 0; r < kn; ++r) {
      float sdot = 0.f, pdot = 0.f;
      for (int d = 0; d < D; ++d) {
        sdot = fmaf(q[d], Kt[r][d], sdot);
        pdot = fmaf(g[d], Vt[r][d], pdot);
      }
      const float p = __expf(sdot * scale - slope * fabsf(qp - kpos[r]) - L);
      const float dsv = p * (pdot - dl) * scale;
      for (int d = 0; d < D; ++d) dq[d] = fmaf(dsv, Kt[r][d], dq[d]);
    }
  }
  if (qi < len) {
    float* row = dqkv + qrow * ld + h * D;
    for (int d = 0; d < D; ++d) row[d] = dq[d];
  }
}

__global__ __launch_bounds__(64) void dkdv_f32_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ cu,
    const int* __restrict__ positions, const float* __restrict__ slopes, int ntile, int total,
    int H, float scale, float* __restrict__ dqkv) {
  __shared__ float Qt[TILE][D + 1], Gt[TILE][D + 1];
  __shared__ float qpos[TILE], Lt[TILE], Dt[TILE];
  Tile t;
  if (!decode(cu, ntile, t)) return;
  const int lane = threadIdx.x, len = t.len, h = t.h;
  const size_t ld = (size_t)3 * H * D;
  const float slope = slopes[h];
  const int kj = t.t0 + lane, kc = min(kj, len - 1);
  const size_t krow = grow(t.cu0, kc, total);
  const float kp = position_of(positions, krow, kc);
  float k[D], v[D], dk[D], dv[D];
  for (int d = 0; d < D; ++d) {
    k[d] = qkv[krow * ld + (size_t)H * D + h * D + d];
    v[d] = qkv[krow * ld + (size_t)2 * H * D + h * D + d];
    dk[d] = dv[d] = 0.f;
  }
  for (int q0 = 0; q0 < len; q0 += TILE) {
    __syncthreads();
    stage_f32(Qt, Gt, qkv + h * D, ld, dout + h * D, (size_t)H * D, t.cu0, len, q0, total, lane);
    {
      const int qc = min(q0 + lane, len - 1);
      const size_t g = grow(t.cu0, qc, total);
      qpos[lane] = position_of(positions, g, qc);
      Lt[lane] = lse[(size_t)h * total + g];
      Dt[lane] = delta[(size_t)h * total + g];
    }
    __syncthreads();
    const int qn = min(TILE, len - q0);
    for (int r = 0; r < qn; ++r) {
      float sdot = 0.f, pdot = 0.f;
      for (int d = 0; d < D; ++d) {
        sdot = fmaf(Qt[r][d], k[d], sdot);
        pdot = fmaf(Gt[r][d], v[d], pdot);
      }
      const float p = __expf(sdot * scale - slope * fabsf(qpos[r] - kp) - Lt[r]);
      const float dsv = p * (pdot - Dt[r]) * scale;
      for (int d = 0; d < D; ++d) {
        dv[d] = fmaf(p, Gt[r][d], dv[d]);
        dk[d] = fmaf(dsv, Qt[r][d], dk[d]);
      }
    }
  }
  if (kj < len) {
    float* row = dqkv + krow * ld + h * D;
    for (int d = 0; d < D; ++d) {
      row[(size_t)H * D + d] = dk[d];
      row[(size_t)2 * H * D + d] = dv[d];
    }
  }
}

}  // namespace attn_varlen
}  // namespace dna

using namespace dna;
using namespace dna::attn_varlen;

static int check_common(const void* qkv, const int* cu, const float* slopes, int nseq,
                        int total_rows, int max_seqlen, int heads, int head_dim, int dtype,
                        const char* fn) {
  DNA_CHECK_ARG(qkv && cu && slopes, "%s: null pointer", fn);
  DNA_CHECK_ARG(nseq > 0 && total_rows > 0 && max_seqlen > 0 && heads > 0,
                "%s: bad shape nseq=%d total_rows=%d max_seqlen=%d heads=%d", fn, nseq, total_rows,
                max_seqlen, heads);
  if (head_dim != D) {
    set_error("%s: head_dim %d unsupported (64 only)", fn, head_dim);
    return DNA_ERR_UNSUPPORTED;
  }
  DNA_CHECK_ARG(dtype == DNA_F32 || dtype == DNA_BF16, "%s: bad dtype %d", fn, dtype);
  const long long tiles = (long long)nseq * ((max_seqlen + TILE - 1) / TILE);
  DNA_CHECK_ARG(tiles <= 0x7fffffffLL && heads <= 65535,
                "%s: grid too large (nseq=%d max_seqlen=%d heads=%d)", fn, nseq, max_seqlen, heads);
  return DNA_OK;
}

extern "C" int dna_attn_varlen_fwd(const void* qkv, const int* cu_seqlens, const int* positions,
                                   const float* slopes, int nseq, int total_rows, int max_seqlen,
                                   int heads, int head_dim, int dtype, float softmax_scale,
                                   void* out, float* lse, void* stream) {
  int st = check_common(qkv, cu_seqlens, slopes, nseq, total_rows, max_seqlen, heads, head_dim,
                        dtype, "dna_attn_varlen_fwd");
  if (st) return st;
  DNA_CHECK_ARG(out && lse, "dna_attn_varlen_fwd: null output");
  hipStream_t s = as_stream(stream);
  const int ntile = (max_seqlen + TILE - 1) / TILE;
  const dim3 grid(nseq * ntile, heads);
  if (dtype == DNA_BF16)
    hipLaunchKernelGGL(fwd_bf16_kernel, grid, dim3(64), 0, s, (const bf16*)qkv, cu_seqlens,
                       positions, slopes, ntile, total_rows, heads, softmax_scale * LOG2E,
                       (bf16*)out, lse);
  else
    hipLaunchKernelGGL(fwd_f32_kernel, grid, dim3(64), 0, s, (const float*)qkv, cu_seqlens,
                       positions, slopes, ntile, total_rows, heads, softmax_scale, (float*)out, lse);
  DNA_LAUNCH_CHECK("dna_attn_varlen_fwd");
  return DNA_OK;
}

extern "C" size_t dna_attn_varlen_bwd_workspace(int nseq, int total_rows, int max_seqlen,
                                                int heads) {
  if (nseq <= 0 || total_rows <= 0 || max_seqlen <= 0 || heads <= 0) return 0;
  return (size_t)heads * total_rows * sizeof(float);  // delta = rowsum(dO * O), [heads, total_rows]
}

extern "C" int dna_attn_varlen_bwd(const void* qkv, const void* out, const void* dout,
                                   const float* lse, const int* cu_seqlens, const int* positions,
                                   const float* slopes, int nseq, int total_rows, int max_seqlen,
                                   int heads, int head_dim, int dtype, float softmax_scale,
                                   void* dqkv, void* workspace, void* stream) {
  int st = check_common(qkv, cu_seqlens, slopes, nseq, total_rows, max_seqlen, heads, head_dim,
                        dtype, "dna_attn_varlen_bwd");
  if (st) return st;
  DNA_CHECK_ARG(out && dout && lse && dqkv, "dna_attn_varlen_bwd: null pointer");
  DNA_CHECK_ARG(workspace && aligned(workspace, 4), "dna_attn_varlen_bwd: null or unaligned workspace");
  hipStream_t s = as_stream(stream);
  float* delta = (float*)workspace;
  const int ntile = (max_seqlen + TILE - 1) / TILE;
  const dim3 grid(nseq * ntile, heads);
  if (dtype == DNA_BF16) {
    hipLaunchKernelGGL(dq_bf16_kernel, grid, dim3(64), 0, s, (const bf16*)qkv, (const bf16*)out,
                       (const bf16*)dout, lse, delta, cu_seqlens, positions, slopes, ntile,
                       total_rows, heads, softmax_scale * LOG2E, softmax_scale, (bf16*)dqkv);
    hipLaunchKernelGGL(dkdv_bf16_kernel, grid, dim3(64), 0, s, (const bf16*)qkv, (const bf16*)dout,
                       lse, delta, cu_seqlens, positions, slopes, ntile, total_rows, heads,
                       softmax_scale * LOG2E, softmax_scale, (bf16*)dqkv);
  } else {
    const size_t n = (size_t)total_rows * heads;
    hipLaunchKernelGGL(delta_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const float*)out, (const float*)dout, total_rows, heads, delta);
    hipLaunchKernelGGL(dq_f32_kernel, grid, dim3(64), 0, s, (const float*)qkv, (const float*)dout,
                       lse, delta, cu_seqlens, positions, slopes, ntile, total_rows, heads,
                       softmax_scale, (float*)dqkv);
    hipLaunchKernelGGL(dkdv_f32_kernel, grid, dim3(64), 0, s, (const float*)qkv,
                       (const float*)dout, lse, delta, cu_seqlens, positions, slopes, ntile,
                       total_rows, heads, softmax_scale, (float*)dqkv);
  }
  DNA_LAUNCH_CHECK("dna_attn_varlen_bwd");
  return DNA_OK;
}
