// Pooling classification head of the HyenaDNA / Caduceus downstream models (reference
// src/tasks/decoders.py SequenceDecoder mode pool / first / last, caduceus
// modeling_caduceus.py:476-620 pooling + score): a windowed mean over L of [B, L, D] hidden
// states, a tiny linear, the loss, and the backward that broadcasts one row per sequence over L.
//
//   m1_b   = (1 / count_b) sum_{l in [start_b, start_b + count_b)} x1[b, l, :]
//   pooled = m1            or, with x2, (m1 + m2) / 2   (m2 over x2, channels reversed if flip2;
//            its window mirrored to [L - start - count, L - start) if flip2 also flips the sequence)
//   logits = pooled W^T (+ bias)
//   g_b = dlogits_b W;  dx[b, l, :] = g_b / count_b (/ 2 with x2) inside the window, 0 outside
//
// Bandwidth-bound: x is read once, dx is written once, 16 bytes per lane and access when D, the
// strides and the pointers allow it (VEC = 4 fp32 / 8 bf16 channels per lane, else VEC = 1 in the
// same kernels). fp32 accumulation in a fixed order, no atomics, no hand-off between workgroups
// inside a launch: bit-identical from run to run.
//
// Forward: partial_kernel sums a chunk of positions per workgroup into part[B][chunks][Dp]
// (chunking from B, L and D, so that B = 1 still fills the device); a lane adds its positions, eight
// loads in flight, into four independent accumulators combined as (a0 + a1) + (a2 + a3), the
// workgroup's position slices are added in slice order. finish_kernel (a workgroup per sequence) adds the chunks in index
// order within each of its chunk groups and the groups in index order, divides by the count,
// writes pooled and computes the logits; loss_kernel is dna_cls_loss's losses with the row
// arithmetic in double (one workgroup).
// Backward: grad_kernel (g, dW, dbias), then bcast_kernel writes every element of dx once.
//
// These kernels take up to 64 labels. The wide head (dna_pool_head_wide_*: up to 1024 labels,
// regression and multi-label) shares partial_kernel and bcast_kernel and has its own stages in
// between; see "the wide head" below.
#include <type_traits>

#include "cls_loss.h"
#include "common.h"

namespace dna {
namespace pool {

constexpr int TPB = 256;  // threads per workgroup of the two whole-tensor kernels

// window of sequence b, clamped to the row: [st, st + cnt) inside [0, L)
__device__ __forceinline__ void window(const int32_t* start, const int32_t* count, int b, int L,
                                       int& st, int& cnt) {
  st = start ? min(max(start[b], 0), L) : 0;
  cnt = count ? min(max(count[b], 0), L - st) : L - st;
}

// VEC consecutive elements at element index idx of an fp32 or bf16 array, as fp32; REV: in
// reverse order (the channel flip of the reverse-complement half)
template <bool BF, int VEC, bool REV>
__device__ __forceinline__ void ldv(const void* p, int64_t idx, float (&o)[VEC]) {
  if constexpr (VEC == 1) {
    o[0] = BF ? (float)reinterpret_cast<const bf16*>(p)[idx] : reinterpret_cast<const float*>(p)[idx];
  } else if constexpr (BF) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(p) + idx);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)v[REV ? 7 - i : i];
  } else {
    const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + idx);
    if constexpr (REV) { o[0] = v.w; o[1] = v.z; o[2] = v.y; o[3] = v.x; }
    else { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
  }
}

template <bool BF, int VEC>
__device__ __forceinline__ void stv(void* p, int64_t idx, const float (&o)[VEC]) {
  if constexpr (VEC == 1) {
    if constexpr (BF) reinterpret_cast<bf16*>(p)[idx] = (bf16)o[0];
    else reinterpret_cast<float*>(p)[idx] = o[0];
  } else if constexpr (BF) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)o[i];
    *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(p) + idx) = v;
  } else {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + idx) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// How the two whole-tensor kernels cut [B, L, D]: a workgroup is cgw lanes over channel vectors
// times TPB / cgw position slices, and owns chunk_len positions of one sequence and column tile.
struct Plan {
  int vec, cgw_log2, coltiles, chunk_len, nchunks;
};

static int pool_chunk_len(int B, int L, int D) {
  // enough workgroups for the device when B is small (2048 over B sequences, at most 512 chunks
  // for the finish kernel), but no chunk so short that a workgroup moves under ~32 KiB
  const int want = min(512, max(1, (2048 + B - 1) / B));
  const int min_len = min(4096, max(32, 16384 / D));
  int64_t len = ((int64_t)L + want - 1) / want;
  if (len < min_len) len = min_len;
  len = (len + 31) / 32 * 32;
  const int64_t whole = ((int64_t)L + 31) / 32 * 32;
  return (int)(len < whole ? len : whole);
}
static int pool_nchunks(int B, int L, int D) {
  const int len = pool_chunk_len(B, L, D);
  return (L + len - 1) / len;
}
static int pool_dp(int D) { return (D + 3) / 4 * 4; }  // row pitch of the fp32 workspaces

static Plan make_plan(int B, int L, int D, int vec) {
  Plan p;
  p.vec = vec;
  const int ncg = (D + vec - 1) / vec;
  p.cgw_log2 = 0;
  while ((1 << p.cgw_log2) < ncg && p.cgw_log2 < 8) ++p.cgw_log2;
  p.coltiles = (ncg + (1 << p.cgw_log2) - 1) >> p.cgw_log2;
  p.chunk_len = pool_chunk_len(B, L, D);
  p.nchunks = pool_nchunks(B, L, D);
  return p;
}

// ------------------------------------------------------------------ forward: partial sums over L
struct PartArgs {
  const void* x1; int64_t s1;
  const void* x2; int64_t s2; int flip2, mirror2;
  const int32_t* start; const int32_t* count;
  int L, D, Dp, cgw_log2, chunk_len, nchunks;
  float* part;  // [B][nchunks][Dp]
};

// acc += the lane's positions lo + rs, lo + rs + RS, ... < hi of one input (channels c .. c + VEC):
// eight positions in flight, added in pairs into four running sums
template <bool BF, int VEC, bool REV>
__device__ __forceinline__ void accumulate(const void* x, int64_t stride, int64_t row0, int c,
                                           int64_t lo, int64_t hi, int rs, int RS,
                                           float (&acc)[4][VEC]) {
  int64_t l = lo + rs;
  for (; l + 7 * RS < hi; l += 8 * RS) {
    float a[8][VEC];
#pragma unroll
    for (int u = 0; u < 8; ++u) ldv<BF, VEC, REV>(x, (row0 + l + u * RS) * stride + c, a[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[u][v] += a[u][v] + a[u + 4][v];
  }
  for (int u = 0; l < hi; l += RS, ++u) {  // at most seven positions left
    float a[VEC];
    ldv<BF, VEC, REV>(x, (row0 + l) * stride + c, a);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      // acc[u & 3][v] with a run-time u would put acc in indexed storage
      if ((u & 3) == 0) acc[0][v] += a[v];
      else if ((u & 3) == 1) acc[1][v] += a[v];
      else if ((u & 3) == 2) acc[2][v] += a[v];
      else acc[3][v] += a[v];
    }
  }
}

template <bool BF, int VEC>
__global__ __launch_bounds__(TPB) void partial_kernel(PartArgs g) {
  __shared__ float red[TPB][VEC + 1];
  const int tid = threadIdx.x;
  const int cgw = 1 << g.cgw_log2, RS = TPB >> g.cgw_log2;
  const int cg = tid & (cgw - 1), rs = tid >> g.cgw_log2;
  const int chunk = blockIdx.x % g.nchunks, ct = blockIdx.x / g.nchunks, b = blockIdx.y;
  const int c0 = ((ct << g.cgw_log2) + cg) * VEC;
  const bool cok = c0 < g.D;  // VEC > 1: D % VEC == 0, the whole vector is inside
  int st, cnt;
  window(g.start, g.count, b, g.L, st, cnt);
  const int64_t c_lo = (int64_t)chunk * g.chunk_len, c_hi = c_lo + g.chunk_len;

  float acc[4][VEC];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[u][v] = 0.f;

  if (cok) {
    const int64_t row0 = (int64_t)b * g.L;
    accumulate<BF, VEC, false>(g.x1, g.s1, row0, c0, max(c_lo, (int64_t)st),
                               min(c_hi, (int64_t)st + cnt), rs, RS, acc);
    if (g.x2) {  // the second input's positions follow in the same running sums
      const int st2 = g.mirror2 ? g.L - st - cnt : st;
      const int64_t lo2 = max(c_lo, (int64_t)st2), hi2 = min(c_hi, (int64_t)st2 + cnt);
      if (g.flip2)  // this lane's outputs c0 .. are x2's channels D - 1 - c0 .. downwards
        accumulate<BF, VEC, true>(g.x2, g.s2, row0, g.D - c0 - VEC, lo2, hi2, rs, RS, acc);
      else
        accumulate<BF, VEC, false>(g.x2, g.s2, row0, c0, lo2, hi2, rs, RS, acc);
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) red[tid][v] = (acc[0][v] + acc[1][v]) + (acc[2][v] + acc[3][v]);
  __syncthreads();
  if (rs == 0 && cok) {  // the position slices, in slice order
    float s[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) s[v] = red[cg][v];
    for (int r = 1; r < RS; ++r)
#pragma unroll
      for (int v = 0; v < VEC; ++v) s[v] += red[(r << g.cgw_log2) + cg][v];
    float* o = g.part + ((int64_t)b * g.nchunks + chunk) * g.Dp + c0;
    if constexpr (VEC == 1) {
      o[0] = s[0];
    } else {
#pragma unroll
      for (int v = 0; v < VEC; v += 4)
        *reinterpret_cast<float4*>(o + v) = make_float4(s[v], s[v + 1], s[v + 2], s[v + 3]);
    }
  }
}

// ------------------------------------------------------------- forward: chunks -> pooled, logits
struct FinArgs {
  const float* part; int nchunks, L, D, Dp, C, cw_log2, two;
  const int32_t* start; const int32_t* count;
  const float* W; const float* bias;
  float* pooled; float* logits;
};

// The pooled row of sequence b from its chunks, by a workgroup of 1024 threads = cw columns (of
// four channels) x 1024 / cw chunk groups. A thread adds its group's chunks in index order (16-B
// loads, eight in flight), then the groups are added in index order through LDS. Ends behind a
// workgroup barrier: every thread may read the row of pooled it wrote.
__device__ __forceinline__ void pooled_row(const FinArgs& g, int b, float4 (&red)[1024]) {
  const int tid = threadIdx.x;
  const int cw = 1 << g.cw_log2, ngroups = 1024 >> g.cw_log2;
  const int col = tid & (cw - 1), grp = tid >> g.cw_log2;
  const int n4 = g.Dp >> 2;
  const int per = (g.nchunks + ngroups - 1) / ngroups;
  int st, cnt;
  window(g.start, g.count, b, g.L, st, cnt);
  const float denom = (float)cnt * (g.two ? 2.f : 1.f);
  const float4* part4 = reinterpret_cast<const float4*>(g.part) + (int64_t)b * g.nchunks * n4;
  for (int cb = 0; cb < n4; cb += cw) {
    const int c4 = cb + col;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < n4) {
      const int q1 = min((grp + 1) * per, g.nchunks);
#pragma unroll 8
      for (int q = grp * per; q < q1; ++q) {
        const float4 v = part4[(int64_t)q * n4 + c4];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
    }
    red[tid] = s;
    __syncthreads();
    if (grp == 0 && c4 < n4) {
      float4 t = red[col];
      for (int u = 1; u < ngroups; ++u) {
        const float4 v = red[(u << g.cw_log2) + col];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
      const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)  // the pad channels D .. Dp - 1 hold nothing
        if (c4 * 4 + k < g.D) g.pooled[(int64_t)b * g.D + c4 * 4 + k] = cnt > 0 ? tv[k] / denom : 0.f;
    }
    __syncthreads();  // red is reused; pooled is read by other threads of this workgroup
  }
}

// One workgroup per sequence: its pooled row, then a wave per class takes the dot product with W
// (lanes stride over D, fixed shuffle tree).
__global__ __launch_bounds__(1024) void finish_kernel(FinArgs g) {
  __shared__ float4 red[1024];
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  pooled_row(g, b, red);
  const float* pb = g.pooled + (int64_t)b * g.D;
  for (int c = w; c < g.C; c += 16) {
    const float* wr = g.W + (int64_t)c * g.D;
    float s = 0.f;
    for (int d = lane; d < g.D; d += 64) s = fmaf(pb[d], wr[d], s);
    s = wave_sum(s);
    if (lane == 0) g.logits[(int64_t)b * g.C + c] = s + (g.bias ? g.bias[c] : 0.f);
  }
}

// ------------------------------------------------------------------------------- forward: loss
// dna_cls_loss's three losses (same labels, same outputs, same tie rule for pred) with the row
// arithmetic in double (cls_loss.h), one workgroup
__global__ __launch_bounds__(1024) void loss_kernel(const float* logits, const void* labels,
                                                    int problem, int B, int C, float* loss,
                                                    float* dlogits, int64_t* pred) {
  cls_loss<double>(logits, labels, problem, B, C, loss, dlogits, pred);
}

// ------------------------------------------------------------------------------------ backward
struct GradArgs {
  const float* dl; const float* upstream; const float* pooled; const float* W;
  const int32_t* start; const int32_t* count;
  int B, L, D, Dp, C, two;
  float* gs;  // [B][Dp]: g_b / count_b (/ 2), what the broadcast stores
  float* dW; float* dbias; int accumulate;
  int blocks_g, blocks_w;
};

// One launch, three kinds of workgroup: gs (an element per thread, the sum over C in class
// order), dW (an element per thread, the sum over B in batch order), dbias (the last workgroup).
__global__ __launch_bounds__(256) void grad_kernel(GradArgs g) {
  const float up = g.upstream ? g.upstream[0] : 1.f;
  int bid = blockIdx.x;
  if (bid < g.blocks_g) {
    const int64_t idx = (int64_t)bid * 256 + threadIdx.x;
    if (idx >= (int64_t)g.B * g.D) return;
    const int b = (int)(idx / g.D), d = (int)(idx - (int64_t)b * g.D);
    int st, cnt;
    window(g.start, g.count, b, g.L, st, cnt);
    float s = 0.f;
    for (int c = 0; c < g.C; ++c) s = fmaf(g.dl[(int64_t)b * g.C + c], g.W[(int64_t)c * g.D + d], s);
    const float denom = (float)cnt * (g.two ? 2.f : 1.f);
    g.gs[(int64_t)b * g.Dp + d] = cnt > 0 ? s * up / denom : 0.f;
    return;
  }
  bid -= g.blocks_g;
  if (bid < g.blocks_w) {
    const int64_t idx = (int64_t)bid * 256 + threadIdx.x;
    if (idx >= (int64_t)g.C * g.D) return;
    const int c = (int)(idx / g.D), d = (int)(idx - (int64_t)c * g.D);
    float s = 0.f;
#pragma unroll 4
    for (int b = 0; b < g.B; ++b) s = fmaf(g.dl[(int64_t)b * g.C + c], g.pooled[(int64_t)b * g.D + d], s);
    g.dW[idx] = g.accumulate ? g.dW[idx] + s * up : s * up;
    return;
  }
  const int c = threadIdx.x;
  if (!g.dbias || c >= g.C) return;
  double s = 0.0;  // a sum of B values that mostly cancel
  for (int b = 0; b < g.B; ++b) s += (double)g.dl[(int64_t)b * g.C + c];
  const float sv = (float)(s * (double)up);
  g.dbias[c] = g.accumulate ? g.dbias[c] + sv : sv;
}

struct BcastArgs {
  const float* gs;
  void* dx1; int64_t s1;
  void* dx2; int64_t s2; int flip2, mirror2;
  const int32_t* start; const int32_t* count;
  int L, D, Dp, cgw_log2, chunk_len, nchunks;
};

// The forward's cut of [B, L, D]: a lane keeps its channels of gs in registers and stores them at
// every position of its slice, zeros outside the window. Every element of dx1 (and dx2) is
// written exactly once.
template <bool BF, int VEC>
__global__ __launch_bounds__(TPB) void bcast_kernel(BcastArgs g) {
  const int tid = threadIdx.x;
  const int cgw = 1 << g.cgw_log2, RS = TPB >> g.cgw_log2;
  const int cg = tid & (cgw - 1), rs = tid >> g.cgw_log2;
  const int chunk = blockIdx.x % g.nchunks, ct = blockIdx.x / g.nchunks, b = blockIdx.y;
  const int c0 = ((ct << g.cgw_log2) + cg) * VEC;
  if (c0 >= g.D) return;
  int st, cnt;
  window(g.start, g.count, b, g.L, st, cnt);
  const int64_t w0 = st, w1 = (int64_t)st + cnt;
  const int64_t m0 = g.mirror2 ? g.L - st - cnt : st, m1 = m0 + cnt;  // dx2's window
  const int64_t lo = (int64_t)chunk * g.chunk_len;
  const int64_t hi = min(lo + g.chunk_len, (int64_t)g.L);
  float v1[VEC], v2[VEC];
  const float* gb = g.gs + (int64_t)b * g.Dp;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    v1[v] = gb[c0 + v];
    v2[v] = g.flip2 ? gb[g.D - 1 - c0 - v] : v1[v];  // dx2's channel c takes g's channel D - 1 - c
  }
  const int64_t row0 = (int64_t)b * g.L;
#pragma unroll 4
  for (int64_t l = lo + rs; l < hi; l += RS) {
    const bool in1 = l >= w0 && l < w1, in2 = l >= m0 && l < m1;
    float o1[VEC], o2[VEC];  // selects of values, not of the arrays (indexed storage otherwise)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      o1[v] = in1 ? v1[v] : 0.f;
      o2[v] = in2 ? v2[v] : 0.f;
    }
    stv<BF, VEC>(g.dx1, (row0 + l) * g.s1 + c0, o1);
    if (g.dx2) stv<BF, VEC>(g.dx2, (row0 + l) * g.s2 + c0, o2);
  }
}

// ------------------------------------------------------------------- the wide head (C <= 1024)
// finish_kernel reads all of W once per sequence, loss_kernel is one workgroup with a thread per
// row, grad_kernel's dbias workgroup has a thread per class: none of them scales in C. The wide
// head keeps partial_kernel and bcast_kernel and replaces the stages between them: pooled_kernel
// (pooled_row alone), three small products on one 32 x 32 tile routine (logits, gs, dW) that read
// each operand once per 32 rows of the other, 128 reduction indices per step, the loss spread over the grid, dbias by column
// slices. The products accumulate in double in index order, so each output carries one rounding.

__global__ __launch_bounds__(1024) void pooled_kernel(FinArgs g) {
  __shared__ float4 red[1024];
  pooled_row(g, blockIdx.x, red);
}

constexpr int TILE = 32;   // rows and columns of a workgroup's tile (256 threads)
constexpr int KSTEP = 128;  // reduction indices staged per step: 16 + 16 loads in flight per thread

struct TileLds {
  float a[KSTEP][TILE + 1], b[KSTEP][TILE + 1];
};

// one operand's [KSTEP][TILE] tile: element (r, k) of the tile is P[(r0 + r) * ld + k0 + k], or
// P[(k0 + k) * ld + r0 + r] when T
template <bool T>
__device__ __forceinline__ void stage_tile(const float* P, int64_t ld, int R, int K, int r0, int k0,
                                           float (&s)[KSTEP][TILE + 1]) {
  const int tid = threadIdx.x;
  constexpr int PER = KSTEP * TILE / 256;
  float v[PER];
  // every load is issued, at a clamped index, before the first value is used: a load under its
  // bounds test waits for the one before it
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int r = T ? (tid & (TILE - 1)) : (tid >> 7) + 2 * u;
    const int k = T ? (tid >> 5) + 8 * u : (tid & (KSTEP - 1));
    const bool ok = r0 + r < R && k0 + k < K;
    const int64_t at = T ? (int64_t)(k0 + k) * ld + r0 + r : (int64_t)(r0 + r) * ld + k0 + k;
    v[u] = P[ok ? at : 0];
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int r = T ? (tid & (TILE - 1)) : (tid >> 7) + 2 * u;
    const int k = T ? (tid >> 5) + 8 * u : (tid & (KSTEP - 1));
    s[k][r] = (r0 + r < R && k0 + k < K) ? v[u] : 0.f;
  }
}

// acc[i][j] = sum_k a(m0 + 2 ty + i, k) b(k, n0 + 2 tx + j) over k = 0 .. K - 1 in index order,
// for the 256 threads (tx = tid % 16, ty = tid / 16) of a workgroup. a(m, k) is A[m * lda + k],
// or A[k * lda + m] when AT; b(k, n) is Bm[n * ldb + k], or Bm[k * ldb + n] when BT. Rows past
// M, columns past N and steps past K read nothing and count as zero. Tiles are staged through
// LDS as [k][m] and [k][n], loaded along the operand's contiguous index.
template <bool AT, bool BT>
__device__ __forceinline__ void tile_product(const float* A, int64_t lda, const float* Bm,
                                             int64_t ldb, int M, int N, int K, int m0, int n0,
                                             TileLds& lds, double (&acc)[2][2]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = 0.0;
  for (int k0 = 0; k0 < K; k0 += KSTEP) {
    stage_tile<AT>(A, lda, M, K, m0, k0, lds.a);
    stage_tile<BT>(Bm, ldb, N, K, n0, k0, lds.b);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < KSTEP; ++k) {
      const double a0 = lds.a[k][2 * ty], a1 = lds.a[k][2 * ty + 1];
      const double b0 = lds.b[k][2 * tx], b1 = lds.b[k][2 * tx + 1];
      acc[0][0] = fma(a0, b0, acc[0][0]);
      acc[0][1] = fma(a0, b1, acc[0][1]);
      acc[1][0] = fma(a1, b0, acc[1][0]);
      acc[1][1] = fma(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
}

// logits = pooled W^T (+ bias): grid (C tiles, B tiles)
__global__ __launch_bounds__(256) void wide_logits_kernel(const float* pooled, const float* W,
                                                          const float* bias, int B, int D, int C,
                                                          float* logits) {
  __shared__ TileLds lds;
  const int m0 = blockIdx.y * TILE, n0 = blockIdx.x * TILE;
  double acc[2][2];
  tile_product<false, false>(pooled, D, W, D, B, C, D, m0, n0, lds, acc);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int b = m0 + 2 * ty + i, c = n0 + 2 * tx + j;
      if (b < B && c < C)
        logits[(int64_t)b * C + c] = (float)(acc[i][j] + (bias ? (double)bias[c] : 0.0));
    }
}

constexpr int LOSS_TPB = 256, LOSS_PER = 2;  // a loss workgroup takes 512 consecutive elements

static int64_t wide_loss_blocks(int B, int C) {
  return ((int64_t)B * C + LOSS_TPB * LOSS_PER - 1) / (LOSS_TPB * LOSS_PER);
}

// cls_loss.h's regression / multi-label element over the B x C elements, an element per thread
// and step, in double; the workgroup's terms are added by a fixed tree into part[blockIdx.x]
__global__ __launch_bounds__(LOSS_TPB) void wide_loss_kernel(const float* logits,
                                                             const float* labels, int problem,
                                                             int64_t n, float* dlogits,
                                                             double* part) {
  __shared__ double red[LOSS_TPB];
  const int tid = threadIdx.x;
  const double inv_n = 1.0 / (double)n;
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < LOSS_PER; ++u) {
    const int64_t i = ((int64_t)blockIdx.x * LOSS_PER + u) * LOSS_TPB + tid;
    if (i < n)
      dlogits[i] = cls_loss_elem<double>(problem, (double)logits[i], (double)labels[i], inv_n, acc);
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = LOSS_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

// loss = (the workgroups' sums, each thread its strided share in index order, then a fixed
// tree) / n; one workgroup
__global__ __launch_bounds__(1024) void wide_loss_finish_kernel(const double* part, int64_t nparts,
                                                                int64_t n, float* loss) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t i = tid; i < nparts; i += 1024) acc += part[i];
  red[tid] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(red[0] / (double)n);
}

// One launch, three kinds of workgroup, as grad_kernel: gs tiles (dlogits W, K = C), dW tiles
// (dlogits^T pooled, K = B), dbias (32 classes x 8 row slices per workgroup: a slice adds its
// rows b = slice, slice + 8, ... in double, the slices are added in slice order).
__global__ __launch_bounds__(256) void wide_grad_kernel(GradArgs g) {
  __shared__ TileLds lds;
  const double up = g.upstream ? (double)g.upstream[0] : 1.0;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int dtiles = (g.D + TILE - 1) / TILE;
  int bid = blockIdx.x;
  double acc[2][2];
  if (bid < g.blocks_g) {
    const int m0 = (bid / dtiles) * TILE, n0 = (bid % dtiles) * TILE;
    tile_product<false, true>(g.dl, g.C, g.W, g.D, g.B, g.D, g.C, m0, n0, lds, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int b = m0 + 2 * ty + i;
      if (b >= g.B) continue;
      int st, cnt;
      window(g.start, g.count, b, g.L, st, cnt);
      const double denom = (double)cnt * (g.two ? 2.0 : 1.0);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int d = n0 + 2 * tx + j;
        if (d < g.D) g.gs[(int64_t)b * g.Dp + d] = cnt > 0 ? (float)(acc[i][j] * up / denom) : 0.f;
      }
    }
    return;
  }
  bid -= g.blocks_g;
  if (bid < g.blocks_w) {
    const int m0 = (bid / dtiles) * TILE, n0 = (bid % dtiles) * TILE;
    tile_product<true, true>(g.dl, g.C, g.pooled, g.D, g.C, g.D, g.B, m0, n0, lds, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = m0 + 2 * ty + i, d = n0 + 2 * tx + j;
        if (c >= g.C || d >= g.D) continue;
        const int64_t idx = (int64_t)c * g.D + d;
        const float sv = (float)(acc[i][j] * up);
        g.dW[idx] = g.accumulate ? g.dW[idx] + sv : sv;
      }
    return;
  }
  bid -= g.blocks_w;
  if (!g.dbias) return;
  __shared__ double col[8][TILE];
  const int cl = tid & (TILE - 1), slice = tid >> 5;
  const int c = bid * TILE + cl;
  double s = 0.0;  // a sum of B values that mostly cancel
  if (c < g.C)
    for (int b = slice; b < g.B; b += 8) s += (double)g.dl[(int64_t)b * g.C + c];
  col[slice][cl] = s;
  __syncthreads();
  if (slice == 0 && c < g.C) {
    for (int u = 1; u < 8; ++u) s += col[u][cl];
    const float sv = (float)(s * up);
    g.dbias[c] = g.accumulate ? g.dbias[c] + sv : sv;
  }
}

// 16-byte accesses when D, the strides and the base pointers allow them, else one element
static int pick_vec(int dtype, int D, const void* p1, int64_t s1, const void* p2, int64_t s2) {
  const int v = dtype == DNA_BF16 ? 8 : 4;
  bool ok = D % v == 0 && s1 % v == 0 && aligned(p1, 16);
  if (p2) ok = ok && s2 % v == 0 && aligned(p2, 16);
  return ok ? v : 1;
}

static int shape_check(const char* name, int B, int L, int D, int C, int dtype, int cmax = 64) {
  DNA_CHECK_ARG(B >= 1 && B <= 65535, "%s: batch must be in [1, 65535] (got %d)", name, B);
  DNA_CHECK_ARG(L >= 1, "%s: length must be >= 1 (got %d)", name, L);
  DNA_CHECK_ARG(D >= 1, "%s: width must be >= 1 (got %d)", name, D);
  DNA_CHECK_ARG(C >= 1 && C <= cmax, "%s: 1 <= labels <= %d required (got %d)", name, cmax, C);
  DNA_CHECK_ARG(dtype == DNA_F32 || dtype == DNA_BF16, "%s: x must be fp32 or bf16", name);
  return DNA_OK;
}

}  // namespace pool
}  // namespace dna

using namespace dna;

// bytes of part[B][nchunks][Dp]; the wide head's loss partial sums (double) follow at a multiple of 16
static size_t part_bytes(int B, int L, int D) {
  const size_t n = (size_t)B * pool::pool_nchunks(B, L, D) * pool::pool_dp(D) * sizeof(float);
  return (n + 15) / 16 * 16;
}

extern "C" size_t dna_pool_head_fwd_workspace(int B, int L, int D) {
  if (B < 1 || L < 1 || D < 1) return 0;
  return (size_t)B * pool::pool_nchunks(B, L, D) * pool::pool_dp(D) * sizeof(float);
}

extern "C" size_t dna_pool_head_wide_fwd_workspace(int B, int L, int D, int C) {
  if (B < 1 || L < 1 || D < 1 || C < 1) return 0;
  return part_bytes(B, L, D) + (size_t)pool::wide_loss_blocks(B, C) * sizeof(double);
}

// Both forwards: partial_kernel, then the narrow head's finish_kernel + loss_kernel or the wide
// head's pooled_kernel + wide_logits_kernel + wide_loss_kernel + wide_loss_finish_kernel.
static int pool_fwd(const char* name, bool wide, const void* x1, int64_t x1_stride, const void* x2,
                    int64_t x2_stride, int flip2, int x_dtype, const int32_t* start,
                    const int32_t* count, const float* W, const float* bias, int B, int L, int D,
                    int C, float* pooled, float* logits, const void* labels, int problem_type,
                    float* loss, float* dlogits, int64_t* pred, void* workspace,
                    size_t workspace_bytes, void* stream) {
  int st = pool::shape_check(name, B, L, D, C, x_dtype, wide ? 1024 : 64);
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(x1 && W && pooled && logits, "%s: null pointer", name);
  DNA_CHECK_ARG((flip2 & ~3) == 0, "%s: bad flip2 flags %d", name, flip2);
  if (labels) {
    DNA_CHECK_ARG(!wide || problem_type != DNA_CLS_SINGLE_LABEL,
                  "%s: problem type single_label_classification is not built for the wide head "
                  "(regression and multi_label_classification are)", name);
    DNA_CHECK_ARG(problem_type == DNA_CLS_REGRESSION || problem_type == DNA_CLS_SINGLE_LABEL ||
                      problem_type == DNA_CLS_MULTI_LABEL,
                  "%s: bad problem type %d", name, problem_type);
    DNA_CHECK_ARG(loss && dlogits, "%s: null loss / dlogits", name);
  }
  DNA_CHECK_ARG(x1_stride >= D && (!x2 || x2_stride >= D), "%s: position strides must be >= D",
                name);
  const size_t need = wide ? dna_pool_head_wide_fwd_workspace(B, L, D, C)
                           : dna_pool_head_fwd_workspace(B, L, D);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need && aligned(workspace, 16),
                "%s: workspace too small or not 16-byte aligned (%zu < %zu)", name,
                workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int vec = pool::pick_vec(x_dtype, D, x1, x1_stride, x2, x2_stride);
  const pool::Plan pl = pool::make_plan(B, L, D, vec);
  const int Dp = pool::pool_dp(D);
  pool::PartArgs pa{x1, x1_stride, x2, x2_stride, x2 && (flip2 & DNA_POOL_FLIP_CHANNELS),
                    x2 && (flip2 & DNA_POOL_MIRROR_WINDOW), start, count, L, D, Dp,
                    pl.cgw_log2, pl.chunk_len, pl.nchunks, (float*)workspace};
  const dim3 grid((unsigned)(pl.nchunks * pl.coltiles), (unsigned)B);
  if (x_dtype == DNA_BF16) {
    if (vec > 1) hipLaunchKernelGGL((pool::partial_kernel<true, 8>), grid, dim3(pool::TPB), 0, s, pa);
    else hipLaunchKernelGGL((pool::partial_kernel<true, 1>), grid, dim3(pool::TPB), 0, s, pa);
  } else {
    if (vec > 1) hipLaunchKernelGGL((pool::partial_kernel<false, 4>), grid, dim3(pool::TPB), 0, s, pa);
    else hipLaunchKernelGGL((pool::partial_kernel<false, 1>), grid, dim3(pool::TPB), 0, s, pa);
  }
  DNA_LAUNCH_CHECK(name);
  int cw_log2 = 0;
  while ((1 << cw_log2) < Dp / 4 && cw_log2 < 8) ++cw_log2;
  pool::FinArgs fa{(const float*)workspace, pl.nchunks, L, D, Dp, C, cw_log2, x2 != nullptr,
                   start, count, W, bias, pooled, logits};
  if (!wide) {
    hipLaunchKernelGGL(pool::finish_kernel, dim3((unsigned)B), dim3(1024), 0, s, fa);
    DNA_LAUNCH_CHECK(name);
    if (labels) {
      hipLaunchKernelGGL(pool::loss_kernel, dim3(1), dim3(1024), 0, s, logits, labels,
                         problem_type, B, C, loss, dlogits, pred);
      DNA_LAUNCH_CHECK(name);
    }
    return DNA_OK;
  }
  hipLaunchKernelGGL(pool::pooled_kernel, dim3((unsigned)B), dim3(1024), 0, s, fa);
  DNA_LAUNCH_CHECK(name);
  const dim3 lgrid((unsigned)((C + pool::TILE - 1) / pool::TILE),
                   (unsigned)((B + pool::TILE - 1) / pool::TILE));
  hipLaunchKernelGGL(pool::wide_logits_kernel, lgrid, dim3(256), 0, s, (const float*)pooled, W,
                     bias, B, D, C, logits);
  DNA_LAUNCH_CHECK(name);
  if (labels) {
    const int64_t n = (int64_t)B * C, nparts = pool::wide_loss_blocks(B, C);
    double* lpart = reinterpret_cast<double*>((char*)workspace + part_bytes(B, L, D));
    hipLaunchKernelGGL(pool::wide_loss_kernel, dim3((unsigned)nparts), dim3(pool::LOSS_TPB), 0, s,
                       (const float*)logits, (const float*)labels, problem_type, n, dlogits, lpart);
    DNA_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(pool::wide_loss_finish_kernel, dim3(1), dim3(1024), 0, s,
                       (const double*)lpart, nparts, n, loss);
    DNA_LAUNCH_CHECK(name);
  }
  return DNA_OK;
}

extern "C" int dna_pool_head_fwd(const void* x1, int64_t x1_stride, const void* x2,
                                 int64_t x2_stride, int flip2, int x_dtype, const int32_t* start,
                                 const int32_t* count, const float* W, const float* bias, int B,
                                 int L, int D, int C, float* pooled, float* logits,
                                 const void* labels, int problem_type, float* loss, float* dlogits,
                                 int64_t* pred, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return pool_fwd("dna_pool_head_fwd", false, x1, x1_stride, x2, x2_stride, flip2, x_dtype, start,
                  count, W, bias, B, L, D, C, pooled, logits, labels, problem_type, loss, dlogits,
                  pred, workspace, workspace_bytes, stream);
}

extern "C" int dna_pool_head_wide_fwd(const void* x1, int64_t x1_stride, const void* x2,
                                      int64_t x2_stride, int flip2, int x_dtype,
                                      const int32_t* start, const int32_t* count, const float* W,
                                      const float* bias, int B, int L, int D, int C, float* pooled,
                                      float* logits, const void* labels, int problem_type,
                                      float* loss, float* dlogits, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return pool_fwd("dna_pool_head_wide_fwd", true, x1, x1_stride, x2, x2_stride, flip2, x_dtype,
                  start, count, W, bias, B, L, D, C, pooled, logits, labels, problem_type, loss,
                  dlogits, nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t dna_pool_head_bwd_workspace(int B, int L, int D) {
  (void)L;
  if (B < 1 || D < 1) return 0;
  return (size_t)B * pool::pool_dp(D) * sizeof(float);
}

extern "C" size_t dna_pool_head_wide_bwd_workspace(int B, int L, int D, int C) {
  return C < 1 ? 0 : dna_pool_head_bwd_workspace(B, L, D);
}

// Both backwards: grad_kernel or wide_grad_kernel (gs, dW, dbias), then bcast_kernel.
static int pool_bwd(const char* name, bool wide, const float* dlogits, const float* upstream,
                    const float* pooled, const float* W, const int32_t* start,
                    const int32_t* count, int B, int L, int D, int C, int x_dtype, void* dx1,
                    int64_t dx1_stride, void* dx2, int64_t dx2_stride, int flip2, float* dW,
                    float* dbias, int accumulate, void* workspace, size_t workspace_bytes,
                    void* stream) {
  int st = pool::shape_check(name, B, L, D, C, x_dtype, wide ? 1024 : 64);
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(dlogits && pooled && W && dW, "%s: null pointer", name);
  DNA_CHECK_ARG(dx1 || !dx2, "%s: dx2 without dx1", name);
  DNA_CHECK_ARG((flip2 & ~3) == 0, "%s: bad flip2 flags %d", name, flip2);
  DNA_CHECK_ARG((!dx1 || dx1_stride >= D) && (!dx2 || dx2_stride >= D),
                "%s: position strides must be >= D", name);
  const size_t need = dna_pool_head_bwd_workspace(B, L, D);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", name,
                workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int Dp = pool::pool_dp(D);
  pool::GradArgs ga{dlogits, upstream, pooled, W, start, count, B, L, D, Dp, C, dx2 != nullptr,
                    (float*)workspace, dW, dbias, accumulate ? 1 : 0, 0, 0};
  if (wide) {
    const int64_t dt = (D + pool::TILE - 1) / pool::TILE, ct = (C + pool::TILE - 1) / pool::TILE;
    const int64_t bg = (B + pool::TILE - 1) / pool::TILE * dt, bw = ct * dt;
    DNA_CHECK_ARG(bg + bw + ct <= INT32_MAX, "%s: width %d makes too many tiles", name, D);
    ga.blocks_g = (int)bg;
    ga.blocks_w = (int)bw;
    hipLaunchKernelGGL(pool::wide_grad_kernel, dim3((unsigned)(bg + bw + ct)), dim3(256), 0, s, ga);
  } else {
    ga.blocks_g = (int)(((int64_t)B * D + 255) / 256);
    ga.blocks_w = (int)(((int64_t)C * D + 255) / 256);
    hipLaunchKernelGGL(pool::grad_kernel, dim3((unsigned)(ga.blocks_g + ga.blocks_w + 1)),
                       dim3(256), 0, s, ga);
  }
  DNA_LAUNCH_CHECK(name);
  if (!dx1) return DNA_OK;  // a frozen backbone: nobody reads dx
  const int vec = pool::pick_vec(x_dtype, D, dx1, dx1_stride, dx2, dx2_stride);
  const pool::Plan pl = pool::make_plan(B, L, D, vec);
  pool::BcastArgs ba{(const float*)workspace, dx1, dx1_stride, dx2, dx2_stride,
                     dx2 && (flip2 & DNA_POOL_FLIP_CHANNELS),
                     dx2 && (flip2 & DNA_POOL_MIRROR_WINDOW), start, count, L, D, Dp, pl.cgw_log2, pl.chunk_len, pl.nchunks};
  const dim3 grid((unsigned)(pl.nchunks * pl.coltiles), (unsigned)B);
  if (x_dtype == DNA_BF16) {
    if (vec > 1) hipLaunchKernelGGL((pool::bcast_kernel<true, 8>), grid, dim3(pool::TPB), 0, s, ba);
    else hipLaunchKernelGGL((pool::bcast_kernel<true, 1>), grid, dim3(pool::TPB), 0, s, ba);
  } else {
    if (vec > 1) hipLaunchKernelGGL((pool::bcast_kernel<false, 4>), grid, dim3(pool::TPB), 0, s, ba);
    else hipLaunchKernelGGL((pool::bcast_kernel<false, 1>), grid, dim3(pool::TPB), 0, s, ba);
  }
  DNA_LAUNCH_CHECK(name);
  return DNA_OK;
}

extern "C" int dna_pool_head_bwd(const float* dlogits, const float* upstream, const float* pooled,
                                 const float* W, const int32_t* start, const int32_t* count, int B,
                                 int L, int D, int C, int x_dtype, void* dx1, int64_t dx1_stride,
                                 void* dx2, int64_t dx2_stride, int flip2, float* dW, float* dbias,
                                 int accumulate, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return pool_bwd("dna_pool_head_bwd", false, dlogits, upstream, pooled, W, start, count, B, L, D,
                  C, x_dtype, dx1, dx1_stride, dx2, dx2_stride, flip2, dW, dbias, accumulate,
                  workspace, workspace_bytes, stream);
}

extern "C" int dna_pool_head_wide_bwd(const float* dlogits, const float* upstream,
                                      const float* pooled, const float* W, const int32_t* start,
                                      const int32_t* count, int B, int L, int D, int C,
                                      int x_dtype, void* dx1, int64_t dx1_stride, void* dx2,
                                      int64_t dx2_stride, int flip2, float* dW, float* dbias,
                                      int accumulate, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return pool_bwd("dna_pool_head_wide_bwd", true, dlogits, upstream, pooled, W, start, count, B, L,
                  D, C, x_dtype, dx1, dx1_stride, dx2, dx2_stride, flip2, dW, dbias, accumulate,
                  workspace, workspace_bytes, stream);
}
