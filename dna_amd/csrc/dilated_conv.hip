// Dense dilated 1-D convolution, channels-last, with the gated-residual epilogues of the
// reference's CNNModel in mode "dilation" (src/models/sequence/denoise.py:468-486), gfx950.
//
//   z[b, l, co] = bias[co] + sum_{t<K} sum_{ci} x[b, l + (t - c) d, ci] * W[co, ci, t],  c = (K-1)/2
//
// as an implicit GEMM with M = B * L rows, N = C and a reduction of K * C: one accumulated
// product per tap over a row-shifted, row-masked A tile. A tile never crosses a sequence (the
// grid's z is the batch index), a shifted row outside [0, L) loads zeros, and a tap whose shifted
// rows all fall outside is skipped (the reference's padding reaches c * d = 256 at d = 64, more
// than a short L: only the centre tap is left then).
//
// bf16 forward / data gradient (fwd_mfma_kernel): 256 threads = 4 waves, a wave owns 32 rows x 64
// output channels = 2 x 4 tiles of v_mfma_f32_16x16x32_bf16, a block 128 rows x 64 channels. The
// operand fragments are 16-B loads straight from memory: a lane's 8 consecutive ci of one
// (shifted) x row, and 8 consecutive ci of one W row of the tap-major weight [K][co][ci]. The
// product is issued swapped (z^T = W x^T), so a lane ends with 4 consecutive co of one row: 8-B
// bf16 / 16-B fp32 epilogue accesses. The epilogue rounds z to the activation dtype and applies
// the layer's combine in place (include/dna_amd.h: DNA_DCONV_*); what it stores is what the
// backward needs -- z_h, g and, for the GELU gate, z_g -- and no [B, L, C] tensor is written only
// to be read back by an elementwise pass.
//
// Weight gradient (wgrad_mfma_kernel): dW_t[co][ci] = sum_rows dz[row][co] x[row + (t-c)d][ci], a
// product that contracts over rows, so both operands are staged as [row][channel] LDS images and
// read with ds_read_b64_tr_b16 (the [k][row] form of csrc/gemm_strided.hip). Block = 64 co x 64 ci
// of one tap and one row range (split); the fp32 partials [split][t][co][ci] and the bias partials
// [split][co] are then summed in split order by reduce_kernel, which also transposes to the
// parameter's [co][ci][t] layout and adds into the flat gradient when asked. No atomics.
//
// fp32: the same ABI on plain FMA kernels (8 interleaved partial sums per tap).
//
// Input layer (onehot_*): Conv1d(V, C, 9) on a one-hot input is a gather from the [V * 9][C] table.
#include "common.h"

namespace dna {
namespace dconv {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ float sigm(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f));
}
__device__ __forceinline__ float apply_act(float z, int act) {
  return act == DNA_ACT_GELU ? gelu_erf(z) : act == DNA_ACT_SIGMOID ? sigm(z) : z;
}
template <typename T> __device__ __forceinline__ float round_to(float v) {
  return to_f32(from_f32<T>(v));
}

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef f32x4 type; };
template <> struct Vec4<bf16> { typedef bf16x4 type; };
template <typename T>
__device__ __forceinline__ void ld4(const T* p, float (&v)[4]) {
  const typename Vec4<T>::type q = *reinterpret_cast<const typename Vec4<T>::type*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (float)q[i];
}
template <typename T>
__device__ __forceinline__ void st4(T* p, const float (&v)[4]) {
  typename Vec4<T>::type q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = (T)v[i];
  *reinterpret_cast<typename Vec4<T>::type*>(p) = q;
}

struct Epi {
  const float* bias;
  const void* g;
  const float* res;
  void* out;
  void* z;
  float* res_out;
  int mode, act;
};

// 4 consecutive output channels co .. co + 3 of one row; idx = the row's offset + co
template <typename T>
__device__ __forceinline__ void epilogue4(const Epi& e, size_t idx, int co, const float (&acc)[4]) {
  float z[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = round_to<T>(acc[i] + (e.bias ? e.bias[co + i] : 0.f));
  if (e.z) st4(reinterpret_cast<T*>(e.z) + idx, z);
  if (e.mode == DNA_DCONV_PLAIN || e.mode == DNA_DCONV_GATE) {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = round_to<T>(apply_act(z[i], e.act));
    st4(reinterpret_cast<T*>(e.out) + idx, o);
    if (e.mode == DNA_DCONV_GATE) {
      float r[4];
      ld4(e.res + idx, r);
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] += o[i];
      st4(e.res_out + idx, r);
    }
    return;
  }
  float g[4], r[4];
  ld4(reinterpret_cast<const T*>(e.g) + idx, g);
  ld4(e.res + idx, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float h = gelu_erf(z[i]);
    r[i] = e.mode == DNA_DCONV_MAIN_MUL ? fmaf(h, g[i], r[i]) : (h + g[i]) + r[i];
  }
  st4(e.res_out + idx, r);
}

// ------------------------------------------------------------------------------- bf16 forward
constexpr int FBM = 128, FBN = 64;

__global__ __launch_bounds__(256) void fwd_mfma_kernel(const bf16* __restrict__ x,
                                                       const bf16* __restrict__ w, Epi e, int L,
                                                       int C, int K, int dil) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, n0 = blockIdx.y * FBN, l0 = blockIdx.x * FBM + wave * 32;
  if (l0 >= L) return;  // no block barrier in this kernel: a wave may leave on its own
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16* xb = x + (size_t)b * L * C;
  const int r = lane & 15, kq = (lane >> 4) * 8, c = (K - 1) / 2;
  for (int t = 0; t < K; ++t) {
    const long long sh = (long long)(t - c) * dil;
    if (l0 + 31 + sh < 0 || l0 + sh >= L) continue;  // the tap is empty for all of this wave's rows
    const bf16* xrow[2];
    bool ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long row = l0 + i * 16 + r + sh;
      ok[i] = row >= 0 && row < L;
      xrow[i] = xb + (size_t)(ok[i] ? row : 0) * C + kq;
    }
    const bf16* wt = w + ((size_t)t * C + n0 + r) * C + kq;
    for (int k0 = 0; k0 < C; k0 += 32) {
      bf16x8 fa[2], fb[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const bf16x8*>(xrow[i] + k0);
        if (!ok[i]) {
#pragma unroll
          for (int q = 0; q < 8; ++q) fa[i][q] = (bf16)0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(wt + (size_t)j * 16 * C + k0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
  }
  // swapped product: the lane holds co = 4 * (lane >> 4) + 0..3 of row lane & 15 of each tile
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int l = l0 + i * 16 + r;
    if (l >= L) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = n0 + j * 16 + 4 * (lane >> 4);
      const float a4[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      epilogue4<bf16>(e, ((size_t)b * L + l) * C + co, co, a4);
    }
  }
}

// ------------------------------------------------------------------------------- fp32 forward
// One thread per 4 output channels co .. co + 3 of one row; a block = 4 rows x 64 such threads.
// Per tap and channel 8 interleaved partial sums over ci, so no sum is longer than C / 8 terms.
__global__ __launch_bounds__(256) void fwd_f32_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ w, Epi e, int L,
                                                      int C, int K, int dil) {
  const int co = (blockIdx.y * 64 + (threadIdx.x & 63)) * 4;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (l >= L || co >= C) return;
  const int c = (K - 1) / 2;
  float tot[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < K; ++t) {
    const long long src = l + (long long)(t - c) * dil;
    if (src < 0 || src >= L) continue;
    const float* xr = x + ((size_t)b * L + src) * C;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float* wr = w + ((size_t)t * C + co + o) * C;
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int ci = 0; ci < C; ci += 8) {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(xr + ci);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(xr + ci + 4);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wr + ci);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(wr + ci + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a[q] = fmaf(x0[q], w0[q], a[q]);
          a[4 + q] = fmaf(x1[q], w1[q], a[4 + q]);
        }
      }
      tot[o] += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
  }
  epilogue4<float>(e, ((size_t)b * L + l) * C + co, co, tot);
}

// ------------------------------------------------------------------------------- backward, elementwise
template <typename T>
__global__ __launch_bounds__(256) void bwd_elem_kernel(const float* __restrict__ dfeat,
                                                       const float* __restrict__ drc,
                                                       const T* __restrict__ zh,
                                                       const T* __restrict__ g,
                                                       const T* __restrict__ zg, size_t n4,
                                                       int forget, T* __restrict__ dzh,
                                                       T* __restrict__ dzg) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const size_t o = i * 4;
    float df[4], dr[4] = {0.f, 0.f, 0.f, 0.f}, z[4], gv[4], zgv[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(dfeat + o, df);
    if (drc) ld4(drc + o, dr);
    ld4(zh + o, z);
    if (forget) ld4(g + o, gv);
    else ld4(zg + o, zgv);
    float oh[4], og[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float h, dh;
      gelu_erf_and_grad(z[q], h, dh);
      if (forget) {
        oh[q] = df[q] * gv[q] * dh;
        og[q] = fmaf(df[q], h, dr[q]) * (gv[q] * (1.f - gv[q]));
      } else {
        oh[q] = df[q] * dh;
        og[q] = (df[q] + dr[q]) * gelu_erf_grad(zgv[q]);
      }
    }
    st4(dzh + o, oh);
    st4(dzg + o, og);
  }
}

// ------------------------------------------------------------------------------- weight gradient
constexpr int WK = 32;      // rows per step
constexpr int WMS = 64 + 8; // [row][channel] image row, elements (144 B: 16-B aligned chunks)

// MFMA operand from a [k][channel] image: channels base + (lane & 15), k = 8 * (lane >> 4) + 0..7
__device__ __forceinline__ bf16x8 frag_t(const bf16* img, int base, int lane) {
  const int i = lane & 15, gq = lane >> 4;
  const bf16* p = img + (8 * gq + (i >> 2)) * WMS + base + 4 * (i & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * WMS));
  return __builtin_bit_cast(bf16x8, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}

// grid (C / 64 co tiles, C / 64 ci tiles, K * splits); part [split][t][co][ci], bpart [split][co]
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(const bf16* __restrict__ dz,
                                                         const bf16* __restrict__ x, int L, int C,
                                                         int K, int dil, long long R,
                                                         long long chunk, int splits,
                                                         float* __restrict__ part,
                                                         float* __restrict__ bpart) {
  __shared__ __attribute__((aligned(16))) bf16 imgA[WK * WMS];
  __shared__ __attribute__((aligned(16))) bf16 imgB[WK * WMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 64;
  const int t = blockIdx.z / splits, sp = blockIdx.z - t * splits;
  const long long sh = (long long)(t - (K - 1) / 2) * dil;
  const bool tap_live = sh > -(long long)L && sh < (long long)L;
  const bool do_bias = bpart && t == 0 && blockIdx.y == 0;
  const long long rb = (long long)sp * chunk;
  const long long re = rb + chunk < R ? rb + chunk : R;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int kk = tid >> 3, ch = (tid & 7) * 8;
  if (tap_live || do_bias) {
    for (long long r0 = rb; r0 < re; r0 += WK) {
      const long long row = r0 + kk;
      bf16x8 va, vb;
#pragma unroll
      for (int q = 0; q < 8; ++q) va[q] = vb[q] = (bf16)0.f;
      if (row < re) {
        va = *reinterpret_cast<const bf16x8*>(dz + (size_t)row * C + co0 + ch);
        const long long l = row % L + sh;
        if (tap_live && l >= 0 && l < L)
          vb = *reinterpret_cast<const bf16x8*>(x + (size_t)(row + sh) * C + ci0 + ch);
      }
      __syncthreads();  // the previous step's fragment reads are done
      *reinterpret_cast<bf16x8*>(imgA + kk * WMS + ch) = va;
      *reinterpret_cast<bf16x8*>(imgB + kk * WMS + ch) = vb;
      __syncthreads();
      if (do_bias && tid < 64) {
#pragma unroll 8
        for (int k = 0; k < WK; ++k) bsum += (float)imgA[k * WMS + tid];
      }
      if (tap_live) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = frag_t(imgA, wm * 32 + i * 16, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = frag_t(imgB, wn * 32 + j * 16, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
      }
    }
  }
  // swapped product: the lane holds ci = 4 * (lane >> 4) + 0..3 of co = lane & 15 of each tile
  float* pt = part + ((size_t)sp * K + t) * C * C;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int co = co0 + wm * 32 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ci = ci0 + wn * 32 + j * 16 + 4 * (lane >> 4);
      *reinterpret_cast<f32x4*>(pt + (size_t)co * C + ci) = acc[i][j];
    }
  }
  if (do_bias && tid < 64) bpart[(size_t)sp * C + co0 + tid] = bsum;
}

// fp32: one thread per (co, ci) of one tap and split, rows in order
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const float* __restrict__ dz,
                                                        const float* __restrict__ x, int L, int C,
                                                        int K, int dil, long long R,
                                                        long long chunk, float* __restrict__ part,
                                                        float* __restrict__ bpart) {
  const int idx = blockIdx.x * 256 + threadIdx.x;  // C * C is a multiple of 256
  const int co = idx / C, ci = idx - co * C;
  const int t = blockIdx.y, sp = blockIdx.z;
  const long long sh = (long long)(t - (K - 1) / 2) * dil;
  const bool tap_live = sh > -(long long)L && sh < (long long)L;
  const bool do_bias = bpart && t == 0 && ci == 0;
  const long long rb = (long long)sp * chunk;
  const long long re = rb + chunk < R ? rb + chunk : R;
  float acc = 0.f, bsum = 0.f;
  if (tap_live || do_bias) {
    for (long long row = rb; row < re; ++row) {
      const float d = dz[(size_t)row * C + co];
      bsum += d;
      const long long l = row % L + sh;
      if (tap_live && l >= 0 && l < L) acc = fmaf(d, x[(size_t)(row + sh) * C + ci], acc);
    }
  }
  part[(((size_t)sp * K + t) * C + co) * C + ci] = acc;
  if (do_bias) bpart[(size_t)sp * C + co] = bsum;
}

// dw[co][ci][t] (+)= sum_split part[split][t][co][ci]; dbias[co] (+)= sum_split bpart[split][co]
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part,
                                                     const float* __restrict__ bpart, int C, int K,
                                                     int splits, int accumulate,
                                                     float* __restrict__ dw,
                                                     float* __restrict__ dbias) {
  const size_t n = (size_t)K * C * C;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += part[(size_t)sp * n + i];
    const size_t t = i / ((size_t)C * C), rem = i - t * (size_t)C * C;  // rem = co * C + ci
    float* o = dw + rem * K + t;
    *o = accumulate ? *o + s : s;
  } else if (dbias && i < n + C) {
    const int co = (int)(i - n);
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += bpart[(size_t)sp * C + co];
    dbias[co] = accumulate ? dbias[co] + s : s;
  }
}

// ------------------------------------------------------------------------------- one-hot input layer
constexpr int OH_MAXV = 8, OH_MAXK = 9;

__device__ __forceinline__ int oh_id(const int64_t* ids, long long pos, int V, int complement) {
  long long id = ids[pos];
  if (complement && id >= 0 && id < 4) id = 3 - id;
  return (id >= 0 && id < V) ? (int)id : -1;
}

// table [v * KW + t][co local] of this block's 64 channels
__device__ __forceinline__ void oh_table(const float* w, int co0, int V, int KW, float* tab) {
  const int VK = V * KW;
  for (int i = threadIdx.x; i < VK * 64; i += blockDim.x) {
    const int col = i / VK, j = i - col * VK;  // consecutive threads read consecutive floats of W
    tab[j * 64 + col] = w[(size_t)(co0 + col) * VK + j];
  }
}

__global__ __launch_bounds__(256) void onehot_fwd_kernel(const int64_t* __restrict__ ids,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ bias, int L,
                                                         long long R, int C, int V, int KW,
                                                         int complement, int act,
                                                         float* __restrict__ out) {
  __shared__ float tab[OH_MAXV * OH_MAXK * 64];
  const int co0 = blockIdx.y * 64, col = threadIdx.x & 63;
  oh_table(w, co0, V, KW, tab);
  __syncthreads();
  const float bc = bias ? bias[co0 + col] : 0.f;
  const int c = (KW - 1) / 2;
  for (int rr = threadIdx.x >> 6; rr < 16; rr += 4) {
    const long long row = (long long)blockIdx.x * 16 + rr;
    if (row >= R) break;
    const int l = (int)(row % L);
    float z = bc;
    for (int t = 0; t < KW; ++t) {
      const int src = l + t - c;
      if (src < 0 || src >= L) continue;
      const int id = oh_id(ids, row + t - c, V, complement);
      if (id >= 0) z += tab[(id * KW + t) * 64 + col];
    }
    out[(size_t)row * C + co0 + col] = act == DNA_ACT_RELU ? fmaxf(z, 0.f) : apply_act(z, act);
  }
}

// grid (splits, C / 64), 64 threads: thread = one channel, rows of the split in order; the
// per-(v, t) sums live in the thread's own LDS column. part [split][co][V * KW + 1] (last: bias).
__global__ __launch_bounds__(64) void onehot_bwd_kernel(const int64_t* __restrict__ ids,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        const float* __restrict__ dout, int L,
                                                        long long R, long long chunk, int C, int V,
                                                        int KW, int complement, int act,
                                                        float* __restrict__ part) {
  __shared__ float tab[OH_MAXV * OH_MAXK * 64];
  __shared__ float sum[OH_MAXV * OH_MAXK * 64];
  const int co0 = blockIdx.y * 64, col = threadIdx.x, VK = V * KW;
  oh_table(w, co0, V, KW, tab);
  for (int j = 0; j < VK; ++j) sum[j * 64 + col] = 0.f;
  __syncthreads();
  const float bc = bias ? bias[co0 + col] : 0.f;
  const int c = (KW - 1) / 2;
  const long long rb = (long long)blockIdx.x * chunk;
  const long long re = rb + chunk < R ? rb + chunk : R;
  float bsum = 0.f;
  for (long long row = rb; row < re; ++row) {
    const int l = (int)(row % L);
    int idt[OH_MAXK];
    float z = bc;
#pragma unroll
    for (int t = 0; t < OH_MAXK; ++t) {
      idt[t] = -1;
      const int src = l + t - c;
      if (t < KW && src >= 0 && src < L) idt[t] = oh_id(ids, row + t - c, V, complement);
      if (idt[t] >= 0) z += tab[(idt[t] * KW + t) * 64 + col];
    }
    float d = dout[(size_t)row * C + co0 + col];
    if (act == DNA_ACT_GELU) d *= gelu_erf_grad(z);
    else if (act == DNA_ACT_SIGMOID) { const float s = sigm(z); d *= s * (1.f - s); }
    else if (act == DNA_ACT_RELU) d = z > 0.f ? d : 0.f;
    bsum += d;
#pragma unroll
    for (int t = 0; t < OH_MAXK; ++t)
      if (idt[t] >= 0) sum[(idt[t] * KW + t) * 64 + col] += d;
  }
  float* p = part + ((size_t)blockIdx.x * C + co0 + col) * (VK + 1);
  for (int j = 0; j < VK; ++j) p[j] = sum[j * 64 + col];
  p[VK] = bsum;
}

__global__ __launch_bounds__(256) void onehot_reduce_kernel(const float* __restrict__ part, int C,
                                                            int VK, int splits, int accumulate,
                                                            float* __restrict__ dw,
                                                            float* __restrict__ dbias) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (co, j), j <= VK
  if (i >= C * (VK + 1)) return;
  const int co = i / (VK + 1), j = i - co * (VK + 1);
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += part[(size_t)sp * C * (VK + 1) + i];
  float* o = j < VK ? dw + (size_t)co * VK + j : (dbias ? dbias + co : nullptr);
  if (o) *o = accumulate ? *o + s : s;
}

}  // namespace dconv
}  // namespace dna

using namespace dna;
using namespace dna::dconv;

static bool shape_ok(int B, int L, int C, int K, int dil) {
  return B > 0 && B <= 65535 && L > 0 && C >= 64 && C <= 512 && C % 64 == 0 && K >= 1 && K <= 9 &&
         (K & 1) && dil >= 1;
}

extern "C" int dna_dconv_fwd(const void* x, int dtype, const void* w_taps, const float* bias, int B,
                             int L, int C, int K, int dilation, int epilogue, int act,
                             const void* g, const float* res, void* out, void* z_out,
                             float* res_out, void* stream) {
  DNA_CHECK_ARG(x && w_taps, "dna_dconv_fwd: null x / w_taps");
  DNA_CHECK_ARG(dtype == DNA_F32 || dtype == DNA_BF16, "dna_dconv_fwd: dtype %d (f32 / bf16)", dtype);
  DNA_CHECK_ARG(shape_ok(B, L, C, K, dilation),
                "dna_dconv_fwd: B=%d L=%d C=%d K=%d dilation=%d unsupported (C %% 64 == 0 in "
                "[64, 512], K odd <= 9, dilation >= 1, B <= 65535)", B, L, C, K, dilation);
  DNA_CHECK_ARG(act == DNA_ACT_NONE || act == DNA_ACT_GELU || act == DNA_ACT_SIGMOID,
                "dna_dconv_fwd: act %d", act);
  switch (epilogue) {
    case DNA_DCONV_PLAIN:
      DNA_CHECK_ARG(out, "dna_dconv_fwd: PLAIN needs out");
      break;
    case DNA_DCONV_GATE:
      DNA_CHECK_ARG(out && res && res_out, "dna_dconv_fwd: GATE needs out, res, res_out");
      break;
    case DNA_DCONV_MAIN_MUL:
    case DNA_DCONV_MAIN_ADD:
      DNA_CHECK_ARG(g && res && res_out && z_out, "dna_dconv_fwd: MAIN_* needs g, res, res_out, z_out");
      break;
    default:
      DNA_CHECK_ARG(false, "dna_dconv_fwd: epilogue %d", epilogue);
  }
  DNA_CHECK_ARG(aligned(x, 16) && aligned(w_taps, 16) && (!g || aligned(g, 16)) &&
                    (!res || aligned(res, 16)) && (!out || aligned(out, 16)) &&
                    (!z_out || aligned(z_out, 16)) && (!res_out || aligned(res_out, 16)) &&
                    (!bias || aligned(bias, 4)),
                "dna_dconv_fwd: pointers must be 16-B aligned");
  const Epi e{bias, g, res, out, z_out, res_out, epilogue, act};
  hipStream_t s = as_stream(stream);
  if (dtype == DNA_BF16) {
    const dim3 grid((L + FBM - 1) / FBM, C / FBN, B);
    hipLaunchKernelGGL(fwd_mfma_kernel, grid, dim3(256), 0, s, (const bf16*)x, (const bf16*)w_taps,
                       e, L, C, K, dilation);
  } else {
    const dim3 grid((L + 3) / 4, (C / 4 + 63) / 64, B);
    hipLaunchKernelGGL(fwd_f32_kernel, grid, dim3(256), 0, s, (const float*)x,
                       (const float*)w_taps, e, L, C, K, dilation);
  }
  DNA_LAUNCH_CHECK("dna_dconv_fwd");
  return DNA_OK;
}

extern "C" int dna_dconv_bwd_elem(const float* dfeat, const float* drc, const void* z_h,
                                  const void* g, const void* z_g, int dtype, size_t n, int forget,
                                  void* dz_h, void* dz_g, void* stream) {
  DNA_CHECK_ARG(dfeat && z_h && dz_h && dz_g && (forget ? g != nullptr : z_g != nullptr),
                "dna_dconv_bwd_elem: null pointer");
  DNA_CHECK_ARG(dtype == DNA_F32 || dtype == DNA_BF16, "dna_dconv_bwd_elem: dtype %d", dtype);
  DNA_CHECK_ARG(n > 0 && n % 4 == 0, "dna_dconv_bwd_elem: n %zu must be a positive multiple of 4", n);
  DNA_CHECK_ARG(aligned(dfeat, 16) && (!drc || aligned(drc, 16)) && aligned(z_h, 8) &&
                    (!g || aligned(g, 8)) && (!z_g || aligned(z_g, 8)) && aligned(dz_h, 8) &&
                    aligned(dz_g, 8),
                "dna_dconv_bwd_elem: misaligned pointer");
  const size_t n4 = n / 4;
  const unsigned blocks = (unsigned)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  hipStream_t s = as_stream(stream);
  if (dtype == DNA_BF16)
    hipLaunchKernelGGL(bwd_elem_kernel<bf16>, dim3(blocks), dim3(256), 0, s, dfeat, drc,
                       (const bf16*)z_h, (const bf16*)g, (const bf16*)z_g, n4, forget, (bf16*)dz_h,
                       (bf16*)dz_g);
  else
    hipLaunchKernelGGL(bwd_elem_kernel<float>, dim3(blocks), dim3(256), 0, s, dfeat, drc,
                       (const float*)z_h, (const float*)g, (const float*)z_g, n4, forget,
                       (float*)dz_h, (float*)dz_g);
  DNA_LAUNCH_CHECK("dna_dconv_bwd_elem");
  return DNA_OK;
}

// Row ranges of the weight gradient: enough (tile, tap, split) blocks to fill the device, at most
// 64, and no range shorter than one 32-row step.
extern "C" int dna_dconv_wgrad_splits(int B, int L, int C, int K) {
  if (!shape_ok(B, L, C, K, 1)) return 0;
  const long long R = (long long)B * L;
  const long long tiles = (long long)(C / 64) * (C / 64) * K;
  long long s = (1024 + tiles - 1) / tiles;
  if (s > 64) s = 64;
  const long long steps = (R + WK - 1) / WK;
  if (s > steps) s = steps;
  return (int)(s < 1 ? 1 : s);
}

extern "C" size_t dna_dconv_wgrad_workspace(int B, int L, int C, int K) {
  const int s = dna_dconv_wgrad_splits(B, L, C, K);
  return (size_t)s * ((size_t)K * C * C + C) * sizeof(float);
}

extern "C" int dna_dconv_wgrad(const void* dz, const void* x, int dtype, int B, int L, int C,
                               int K, int dilation, float* dw, float* dbias, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream) {
  DNA_CHECK_ARG(dz && x && dw && workspace, "dna_dconv_wgrad: null pointer");
  DNA_CHECK_ARG(dtype == DNA_F32 || dtype == DNA_BF16, "dna_dconv_wgrad: dtype %d", dtype);
  DNA_CHECK_ARG(shape_ok(B, L, C, K, dilation),
                "dna_dconv_wgrad: B=%d L=%d C=%d K=%d dilation=%d unsupported", B, L, C, K, dilation);
  DNA_CHECK_ARG(workspace_bytes >= dna_dconv_wgrad_workspace(B, L, C, K),
                "dna_dconv_wgrad: workspace too small");
  DNA_CHECK_ARG(aligned(dz, 16) && aligned(x, 16) && aligned(workspace, 16),
                "dna_dconv_wgrad: pointers must be 16-B aligned");
  const int splits = dna_dconv_wgrad_splits(B, L, C, K);
  const long long R = (long long)B * L;
  long long chunk = (R + splits - 1) / splits;
  chunk = (chunk + WK - 1) / WK * WK;
  float* part = (float*)workspace;
  float* bpart = part + (size_t)splits * K * C * C;
  hipStream_t s = as_stream(stream);
  if (dtype == DNA_BF16) {
    hipLaunchKernelGGL(wgrad_mfma_kernel, dim3(C / 64, C / 64, K * splits), dim3(256), 0, s,
                       (const bf16*)dz, (const bf16*)x, L, C, K, dilation, R, chunk, splits, part,
                       dbias ? bpart : nullptr);
  } else {
    hipLaunchKernelGGL(wgrad_f32_kernel, dim3(C * C / 256, K, splits), dim3(256), 0, s,
                       (const float*)dz, (const float*)x, L, C, K, dilation, R, chunk, part,
                       dbias ? bpart : nullptr);
  }
  DNA_LAUNCH_CHECK("dna_dconv_wgrad");
  const size_t n = (size_t)K * C * C + C;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, bpart,
                     C, K, splits, accumulate, dw, dbias);
  DNA_LAUNCH_CHECK("dna_dconv_wgrad (reduce)");
  return DNA_OK;
}

static bool onehot_ok(int B, int L, int C, int V, int KW) {
  return B > 0 && L > 0 && C >= 64 && C % 64 == 0 && C <= 65535 * 64 && V >= 1 && V <= OH_MAXV &&
         KW >= 1 && KW <= OH_MAXK && (KW & 1);
}

extern "C" int dna_onehot_conv_fwd(const int64_t* ids, const float* w, const float* bias, int B,
                                   int L, int C, int V, int KW, int complement, int act, float* out,
                                   void* stream) {
  DNA_CHECK_ARG(ids && w && out, "dna_onehot_conv_fwd: null pointer");
  DNA_CHECK_ARG(onehot_ok(B, L, C, V, KW),
                "dna_onehot_conv_fwd: B=%d L=%d C=%d V=%d KW=%d unsupported (C %% 64 == 0, V <= 8, "
                "KW odd <= 9)", B, L, C, V, KW);
  DNA_CHECK_ARG(act == DNA_ACT_NONE || act == DNA_ACT_GELU || act == DNA_ACT_SIGMOID ||
                    act == DNA_ACT_RELU,
                "dna_onehot_conv_fwd: act %d", act);
  const long long R = (long long)B * L;
  DNA_CHECK_ARG((R + 15) / 16 < (1ll << 31), "dna_onehot_conv_fwd: too many rows");
  hipLaunchKernelGGL(onehot_fwd_kernel, dim3((unsigned)((R + 15) / 16), C / 64), dim3(256), 0,
                     as_stream(stream), ids, w, bias, L, R, C, V, KW, complement, act, out);
  DNA_LAUNCH_CHECK("dna_onehot_conv_fwd");
  return DNA_OK;
}

static int onehot_splits(int B, int L) {
  const long long R = (long long)B * L;
  const long long s = (R + 63) / 64;
  return (int)(s > 1024 ? 1024 : s);
}

extern "C" size_t dna_onehot_conv_bwd_workspace(int B, int L, int C, int V, int KW) {
  if (!onehot_ok(B, L, C, V, KW)) return 0;
  return (size_t)onehot_splits(B, L) * C * (V * KW + 1) * sizeof(float);
}

extern "C" int dna_onehot_conv_bwd(const int64_t* ids, const float* w, const float* bias,
                                   const float* dout, int B, int L, int C, int V, int KW,
                                   int complement, int act, float* dw, float* dbias, int accumulate,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  DNA_CHECK_ARG(ids && w && dout && dw && workspace, "dna_onehot_conv_bwd: null pointer");
  DNA_CHECK_ARG(onehot_ok(B, L, C, V, KW),
                "dna_onehot_conv_bwd: B=%d L=%d C=%d V=%d KW=%d unsupported", B, L, C, V, KW);
  DNA_CHECK_ARG(act == DNA_ACT_NONE || act == DNA_ACT_GELU || act == DNA_ACT_SIGMOID ||
                    act == DNA_ACT_RELU,
                "dna_onehot_conv_bwd: act %d", act);
  DNA_CHECK_ARG(workspace_bytes >= dna_onehot_conv_bwd_workspace(B, L, C, V, KW),
                "dna_onehot_conv_bwd: workspace too small");
  const int splits = onehot_splits(B, L);
  const long long R = (long long)B * L;
  const long long chunk = (R + splits - 1) / splits;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(onehot_bwd_kernel, dim3(splits, C / 64), dim3(64), 0, s, ids, w, bias, dout, L,
                     R, chunk, C, V, KW, complement, act, (float*)workspace);
  DNA_LAUNCH_CHECK("dna_onehot_conv_bwd");
  const int n = C * (V * KW + 1);
  hipLaunchKernelGGL(onehot_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                     (const float*)workspace, C, V * KW, splits, accumulate, dw, dbias);
  DNA_LAUNCH_CHECK("dna_onehot_conv_bwd (reduce)");
  return DNA_OK;
}
