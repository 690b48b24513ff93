// Masked-LM head for small vocabularies (the HyenaDNA "blm" model with the character tokenizer:
// 12 tokens padded to 16): the tied-weight projection, the cross entropy over the masked rows and
// their backward, without a logits tensor. For hidden states h [T, D], the tied weight W [V, D]
// (V <= 64, no bias) and labels [T] (int64; a row whose label is outside [0, V) is ignored):
//
//   logit_v  = sum_d h[r, d] W[v, d]                       (fp32)
//   loss_r   = lse_r - logit_label,   loss = sum_r loss_r / count      (count = kept rows)
//   coef_r,v = softmax(logit_r)_v - [v == label_r]         (kept rows only)
//   dh[r, :] = g / count * sum_v coef_r,v W[v, :]          (exact zeros on ignored rows)
//   dW[v, :] = g / count * sum_r coef_r,v h[r, :]
//
// Bandwidth-bound: the kept rows of h (15 % of them in BERT masking) are read twice (forward,
// dW), ignored rows never, dh is written once, every element. 16 bytes per lane and access when D,
// the strides and the pointers allow it (VEC = 4 fp32 / 8 bf16), else one element in the same
// kernels. fp32 accumulation in a fixed order, no atomics, no hand-off between workgroups inside a
// launch: bit-identical from run to run.
//
// Forward: rows_kernel, a wave per RPW consecutive rows. A lane reads one label, the ballot of
// kept rows steers the wave; per kept row the lanes split D, V shuffle-tree sums leave logit_v in
// lane v, max / sum / log over the lanes give the row's loss (added in double per wave, waves in
// index order per workgroup), lane v stores coef_r,v for the backward. finish_kernel (one
// workgroup) adds the workgroups' partial sums in a fixed tree: loss_sum, count, loss.
// Backward: dh_kernel (the forward's cut of the rows; lane v holds coef_r,v, the lanes split D),
// dw_part_kernel (a thread per column, a workgroup per chunk of rows: the chunk's kept rows are
// listed in index order, then added in that order), dw_finish_kernel (chunks in index order).
//
// RC-equivariant head (Caduceus RCPSLMHead; dna_lm_head_rc_*): rows of 2 D channels, the tied
// W [V, D] and a complement map cm [V]:
//
//   logit_v = sum_{d<D} h[r, d] W[v, d] + sum_{d<D} h[r, 2D-1-d] W[cm[v], d]
//
// which is the head above over 2 D channels with Wt[v, d] = W[v, d], Wt[v, D + j] =
// W[cm[v], D-1-j]. rc_expand_kernel writes Wt (W's dtype, at most 64 x 2 D elements) into the
// workspace, the five kernels above run unchanged at width 2 D, and rc_fold_kernel takes the
// gradient of Wt back to W: dW[u, d] (+)= dWt[u, d] + sum over v with cm[v] == u, v ascending,
// of dWt[v, 2D-1-d] -- the backward of the gather W[cm], whatever cm is (not an involution, not
// injective), one thread per element, a fixed order, no atomics.
//
// Biased head (the CNN's untied out_linear; dna_lm_head_bias_*): logit_v += bias[v], one fp32 add
// after the row's sum, and dbias[v] = g / count * sum_r coef_r,v. dw_part_kernel takes the bias as
// column D of an h whose extra column is 1: the same chunks, the same lists, the same order; its
// partials go to their own [chunks][V] block and dw_finish_kernel sums them. A null bias runs the
// kernels above exactly as before.
#include <math.h>

#include "common.h"

namespace dna {
namespace lmh {

constexpr int TPB = 256;         // threads per workgroup
constexpr int WAVES = TPB / 64;  // waves per workgroup
constexpr int RPW = 16;          // rows per wave of the row kernels
constexpr int RPB = WAVES * RPW;
constexpr int NCH = 4;           // 64-lane chunks of a row a wave keeps in registers (REG)
constexpr int VG = 8;            // vocabulary entries whose W loads are in flight together

// VEC consecutive elements at element index idx of an fp32 or bf16 array, as fp32
template <bool BF, int VEC>
__device__ __forceinline__ void ldv(const void* p, int64_t idx, float (&o)[VEC]) {
  if constexpr (VEC == 1) {
    o[0] = BF ? (float)reinterpret_cast<const bf16*>(p)[idx] : reinterpret_cast<const float*>(p)[idx];
  } else if constexpr (BF) {
    static_assert(VEC == 4 || VEC == 8, "bf16 vectors of 4 or 8");
    if constexpr (VEC == 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(p) + idx);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
    } else {
      const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(p) + idx);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (float)v[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + idx + i);
      o[i] = v.x; o[i + 1] = v.y; o[i + 2] = v.z; o[i + 3] = v.w;
    }
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

// The labels of the wave's rows base .. base + RPW - 1 (one per lane) -> the label this lane
// read and the mask of kept rows. A label outside [0, V) never indexes W: its row is ignored.
__device__ __forceinline__ uint64_t wave_rows(const int64_t* labels, int64_t base, int T, int V,
                                              int lane, int& label) {
  int64_t y = -1;
  if (lane < RPW && base + lane < T) y = labels[base + lane];
  const bool keep = y >= 0 && y < V;
  label = keep ? (int)y : -1;
  return __ballot(keep);
}

// ------------------------------------------------------------------------------------- forward
struct RowArgs {
  const void* h; int64_t hs; const void* W; const float* bias;  // bias [V] fp32; NULL: none
  const int64_t* labels;
  int T, D, V;
  float* coef;                        // [T][V], kept rows only; NULL: not wanted
  double* part_loss; int64_t* part_cnt;  // [workgroups]
};

// logit_v of one row in lane v (-inf in lanes >= V). REG: D <= NCH * 64 * VEC and the lane's
// elements of the row stay in registers over the V passes; else they are read again per pass
// (L1 hits).
template <bool HBF, bool WBF, int VEC, bool REG>
__device__ __forceinline__ float row_logits(const void* h, int64_t off, const void* W, int D,
                                            int V, int lane) {
  float hr[NCH][VEC];
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int d = (k * 64 + lane) * VEC;
#pragma unroll
      for (int j = 0; j < VEC; ++j) hr[k][j] = 0.f;
      if (d < D) ldv<HBF, VEC>(h, off + d, hr[k]);  // VEC > 1: D % VEC == 0, the vector is inside
    }
  }
  float mine = -INFINITY;
  // VG entries at a time: their W loads (L1 / L2 hits) are issued before the first is used, and
  // the VG shuffle trees are independent of each other; an entry >= V reads row V - 1 again
  for (int v0 = 0; v0 < V; v0 += VG) {
    float s[VG];
#pragma unroll
    for (int u = 0; u < VG; ++u) s[u] = 0.f;
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int d = (k * 64 + lane) * VEC;
        if (d < D) {
          float wv[VG][VEC];
#pragma unroll
          for (int u = 0; u < VG; ++u)
            ldv<WBF, VEC>(W, (int64_t)min(v0 + u, V - 1) * D + d, wv[u]);
#pragma unroll
          for (int u = 0; u < VG; ++u)
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[u] = fmaf(hr[k][j], wv[u][j], s[u]);
        }
      }
    } else {
      for (int d = lane * VEC; d < D; d += 64 * VEC) {
        float hv[VEC], wv[VG][VEC];
        ldv<HBF, VEC>(h, off + d, hv);
#pragma unroll
        for (int u = 0; u < VG; ++u)
          ldv<WBF, VEC>(W, (int64_t)min(v0 + u, V - 1) * D + d, wv[u]);
#pragma unroll
        for (int u = 0; u < VG; ++u)
#pragma unroll
          for (int j = 0; j < VEC; ++j) s[u] = fmaf(hv[j], wv[u][j], s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < VG; ++u) {
      const float t = wave_sum(s[u]);
      if (lane == v0 + u && v0 + u < V) mine = t;
    }
  }
  return mine;
}

template <bool HBF, bool WBF, int VEC, bool REG>
__global__ __launch_bounds__(TPB) void rows_kernel(RowArgs g) {
  __shared__ double sl[WAVES];
  __shared__ int sc[WAVES];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t base = ((int64_t)blockIdx.x * WAVES + w) * RPW;
  int label;
  uint64_t m = wave_rows(g.labels, base, g.T, g.V, lane, label);
  double loss = 0.0;
  int cnt = 0;
  while (m) {
    const int i = __builtin_ctzll(m);
    m &= m - 1;
    const int y = __shfl(label, i);
    const int64_t r = base + i;
    float logit = row_logits<HBF, WBF, VEC, REG>(g.h, r * g.hs, g.W, g.D, g.V, lane);
    if (g.bias && lane < g.V) logit += g.bias[lane];
    const float mx = wave_max(logit);
    const float e = lane < g.V ? expf(logit - mx) : 0.f;
    const float s = wave_sum(e);
    const float ly = __shfl(logit, y);
    loss += (double)mx + (double)logf(s) - (double)ly;
    ++cnt;
    if (g.coef && lane < g.V) g.coef[r * g.V + lane] = e / s - (lane == y ? 1.f : 0.f);
  }
  if (lane == 0) { sl[w] = loss; sc[w] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sl[0];
    int c = sc[0];
    for (int u = 1; u < WAVES; ++u) { a += sl[u]; c += sc[u]; }
    g.part_loss[blockIdx.x] = a;
    g.part_cnt[blockIdx.x] = c;
  }
}

// One workgroup: the partial sums in a fixed order (a thread adds every 1024th, then a tree).
// loss = loss_sum / (denom > 0 ? denom : count), 0 when no row is kept.
__global__ __launch_bounds__(1024) void finish_kernel(const double* part_loss,
                                                      const int64_t* part_cnt, int n, float denom,
                                                      float* loss_sum, int64_t* count, float* loss) {
  __shared__ double rl[1024];
  __shared__ long long rc[1024];
  const int tid = threadIdx.x;
  double a = 0.0;
  long long c = 0;
  for (int i = tid; i < n; i += 1024) { a += part_loss[i]; c += part_cnt[i]; }
  rl[tid] = a;
  rc[tid] = c;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) { rl[tid] += rl[tid + s]; rc[tid] += rc[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    loss_sum[0] = (float)rl[0];
    count[0] = rc[0];
    if (loss) {
      const double dn = denom > 0.f ? (double)denom : (double)rc[0];
      loss[0] = rc[0] > 0 ? (float)(rl[0] / dn) : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------ backward
// upstream / (denom > 0 ? denom : count); 0 when no row is kept
__device__ __forceinline__ float grad_scale(const float* upstream, const int64_t* count,
                                            float denom) {
  const int64_t c = count[0];
  if (c <= 0) return 0.f;
  const float up = upstream ? upstream[0] : 1.f;
  return up / (denom > 0.f ? denom : (float)c);
}

struct DhArgs {
  const float* coef; const void* W; const int64_t* labels; const int64_t* count;
  const float* upstream; float denom;
  int T, D, V;
  void* dh; int64_t ds;
};

// Every element of dh once: sum_v (scale coef_r,v) W[v, :] on kept rows, zeros elsewhere.
template <bool HBF, bool WBF, int VEC>
__global__ __launch_bounds__(TPB) void dh_kernel(DhArgs g) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t base = ((int64_t)blockIdx.x * WAVES + w) * RPW;
  const float scale = grad_scale(g.upstream, g.count, g.denom);
  int label;
  const uint64_t m = wave_rows(g.labels, base, g.T, g.V, lane, label);
  for (int i = 0; i < RPW && base + i < g.T; ++i) {
    const int64_t r = base + i;
    const bool kept = (m >> i) & 1;  // the same in every lane
    float c = 0.f;
    if (kept && lane < g.V) c = g.coef[r * g.V + lane] * scale;
    // every lane runs every pass of both loops (the shuffle reads lane v)
    for (int d0 = 0; d0 < g.D; d0 += 64 * VEC) {
      const int d = d0 + lane * VEC;
      float o[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = 0.f;
      if (kept) {
        // VG entries at a time, their W loads in flight together, added in entry order; an
        // entry >= V reads row V - 1 again with coefficient 0 (lanes >= V hold c = 0)
        for (int v0 = 0; v0 < g.V; v0 += VG) {
          float cv[VG], wv[VG][VEC];
#pragma unroll
          for (int u = 0; u < VG; ++u) {
            cv[u] = v0 + u < g.V ? __shfl(c, min(v0 + u, 63)) : 0.f;
            if (d < g.D) ldv<WBF, VEC>(g.W, (int64_t)min(v0 + u, g.V - 1) * g.D + d, wv[u]);
          }
          if (d < g.D) {
#pragma unroll
            for (int u = 0; u < VG; ++u)
#pragma unroll
              for (int j = 0; j < VEC; ++j) o[j] = fmaf(cv[u], wv[u][j], o[j]);
          }
        }
      }
      if (d < g.D) stv<HBF, VEC>(g.dh, r * g.ds + d, o);
    }
  }
}

struct DwArgs {
  const float* coef; const void* h; int64_t hs; const int64_t* labels;
  int T, D, V, chunk_len;
  float* part;    // [chunks][V][D]
  float* part_b;  // [chunks][V]: the bias column (column D, h = 1); NULL: not wanted
};

// Workgroup (x, y): columns 256 x .. of chunk y's rows. Per 256 rows the kept ones are listed in
// index order (ballot + prefix counts), then a thread adds coef_r,v h[r, d] over the list into
// its V sums; coef_r,: is read through scalar loads (the row is the same in every lane). With
// part_b the grid covers D + 1 columns and column D sums coef_r,v alone (the bias gradient).
template <bool HBF, int VMAX>
__global__ __launch_bounds__(TPB) void dw_part_kernel(DwArgs g) {
  __shared__ int list[TPB];
  __shared__ int wcnt[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int d = blockIdx.x * TPB + tid;
  const int chunk = blockIdx.y;
  const int64_t r0 = (int64_t)chunk * g.chunk_len;
  const int64_t r1 = min(r0 + g.chunk_len, (int64_t)g.T);
  const int ncol = g.part_b ? g.D + 1 : g.D;
  float acc[VMAX];
#pragma unroll
  for (int v = 0; v < VMAX; ++v) acc[v] = 0.f;
  for (int64_t sb = r0; sb < r1; sb += TPB) {
    const int64_t r = sb + tid;
    bool keep = false;
    if (r < r1) {
      const int64_t y = g.labels[r];
      keep = y >= 0 && y < g.V;
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) wcnt[w] = __popcll(b);
    __syncthreads();
    int off = 0, n = 0;
    for (int u = 0; u < WAVES; ++u) {
      if (u < w) off += wcnt[u];
      n += wcnt[u];
    }
    if (keep) list[off + __popcll(b & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    if (d < ncol) {
      // eight listed rows at a time: their loads are issued before the first is used; the
      // sums still take the rows in list order
      for (int i0 = 0; i0 < n; i0 += 8) {
        float hv[8];
        int64_t rr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          rr[u] = sb + __builtin_amdgcn_readfirstlane(list[min(i0 + u, n - 1)]);
          if (d == g.D) hv[u] = 1.f;
          else hv[u] = HBF ? (float)reinterpret_cast<const bf16*>(g.h)[rr[u] * g.hs + d]
                           : reinterpret_cast<const float*>(g.h)[rr[u] * g.hs + d];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (i0 + u < n) {
            const float* c = g.coef + rr[u] * g.V;
#pragma unroll
            for (int v = 0; v < VMAX; ++v)
              if (v < g.V) acc[v] = fmaf(c[v], hv[u], acc[v]);
          }
        }
      }
    }
    __syncthreads();  // list and wcnt are rewritten by the next 256 rows
  }
  if (d < g.D) {
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < g.V) g.part[((int64_t)chunk * g.V + v) * g.D + d] = acc[v];
  } else if (d == g.D && g.part_b) {
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < g.V) g.part_b[(int64_t)chunk * g.V + v] = acc[v];
  }
}

// dW[v, d] (+)= scale * (the chunks' partial sums in index order)
__global__ __launch_bounds__(TPB) void dw_finish_kernel(const float* part, int nchunks, int n,
                                                        const int64_t* count,
                                                        const float* upstream, float denom,
                                                        float* dW, int accumulate) {
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= n) return;
  const float scale = grad_scale(upstream, count, denom);
  float s = 0.f;
#pragma unroll 8
  for (int q = 0; q < nchunks; ++q) s += part[(int64_t)q * n + idx];
  dW[idx] = accumulate ? dW[idx] + s * scale : s * scale;
}

// Wt [V, 2 D] in W's dtype: Wt[v, d] = W[v, d], Wt[v, D + j] = W[cm[v], D-1-j]. The entries of cm
// are validated where the map is built, on the host; one outside [0, V) reads nothing here (0).
template <bool WBF>
__global__ __launch_bounds__(TPB) void rc_expand_kernel(const void* W, const int64_t* cm, int D,
                                                        int V, void* Wt) {
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= V * 2 * D) return;
  const int v = idx / (2 * D), c = idx - v * 2 * D;
  int64_t src;
  if (c < D) {
    src = (int64_t)v * D + c;
  } else {
    const int64_t u = cm[v];
    src = u >= 0 && u < V ? u * D + (2 * D - 1 - c) : -1;
  }
  if constexpr (WBF) {
    reinterpret_cast<bf16*>(Wt)[idx] = src >= 0 ? reinterpret_cast<const bf16*>(W)[src] : (bf16)0.f;
  } else {
    reinterpret_cast<float*>(Wt)[idx] = src >= 0 ? reinterpret_cast<const float*>(W)[src] : 0.f;
  }
}

// dW[u, d] (+)= dWt[u, d] + sum_{v ascending, cm[v] == u} dWt[v, 2D-1-d]; a thread per (u, d)
__global__ __launch_bounds__(TPB) void rc_fold_kernel(const float* dWt, const int64_t* cm, int D,
                                                      int V, float* dW, int accumulate) {
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= V * D) return;
  const int u = idx / D, d = idx - u * D;
  float s = dWt[(int64_t)u * 2 * D + d];
  for (int v = 0; v < V; ++v)
    if (cm[v] == u) s += dWt[(int64_t)v * 2 * D + (2 * D - 1 - d)];
  dW[idx] = accumulate ? dW[idx] + s : s;
}

// pool_head.hip's rule: 16-byte accesses when D, the row stride and the base pointers allow
// them (the rows of the contiguous W are then 16-byte aligned in either dtype), else one element
static int pick_vec(int dtype, int D, const void* p, int64_t stride, const void* W) {
  const int v = dtype == DNA_BF16 ? 8 : 4;
  return D % v == 0 && stride % v == 0 && aligned(p, 16) && aligned(W, 16) ? v : 1;
}

static int dw_chunk_len(int T) {
  // at most 256 chunks (the finish kernel's serial sum), whole 256-row blocks
  const int64_t len = (((int64_t)T + 255) / 256 + 255) / 256 * 256;
  return (int)len;
}
static int dw_nchunks(int T) {
  const int len = dw_chunk_len(T);
  return (int)(((int64_t)T + len - 1) / len);
}
static int row_blocks(int T) { return (int)(((int64_t)T + RPB - 1) / RPB); }

static int shape_check(const char* name, int T, int D, int V, int h_dtype, int w_dtype) {
  DNA_CHECK_ARG(T >= 1, "%s: rows must be >= 1 (got %d)", name, T);
  DNA_CHECK_ARG(D >= 1, "%s: width must be >= 1 (got %d)", name, D);
  DNA_CHECK_ARG(V >= 1 && V <= 64, "%s: 1 <= vocabulary <= 64 required (got %d)", name, V);
  DNA_CHECK_ARG(h_dtype == DNA_F32 || h_dtype == DNA_BF16, "%s: h must be fp32 or bf16", name);
  DNA_CHECK_ARG(w_dtype == DNA_F32 || w_dtype == DNA_BF16, "%s: W must be fp32 or bf16", name);
  return DNA_OK;
}

template <bool HBF, bool WBF>
static void launch_rows(int vec, bool reg, dim3 grid, hipStream_t s, const RowArgs& a) {
  constexpr int VN = HBF ? 8 : 4;
  if (vec > 1) {
    if (reg) hipLaunchKernelGGL((rows_kernel<HBF, WBF, VN, true>), grid, dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL((rows_kernel<HBF, WBF, VN, false>), grid, dim3(TPB), 0, s, a);
  } else {
    if (reg) hipLaunchKernelGGL((rows_kernel<HBF, WBF, 1, true>), grid, dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL((rows_kernel<HBF, WBF, 1, false>), grid, dim3(TPB), 0, s, a);
  }
}

template <bool HBF, bool WBF>
static void launch_dh(int vec, dim3 grid, hipStream_t s, const DhArgs& a) {
  constexpr int VN = HBF ? 8 : 4;
  if (vec > 1) hipLaunchKernelGGL((dh_kernel<HBF, WBF, VN>), grid, dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL((dh_kernel<HBF, WBF, 1>), grid, dim3(TPB), 0, s, a);
}

template <bool HBF>
static void launch_dw(int V, dim3 grid, hipStream_t s, const DwArgs& a) {
  if (V <= 16) hipLaunchKernelGGL((dw_part_kernel<HBF, 16>), grid, dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL((dw_part_kernel<HBF, 64>), grid, dim3(TPB), 0, s, a);
}

}  // namespace lmh
}  // namespace dna

using namespace dna;

extern "C" size_t dna_lm_head_fwd_workspace(int T) {
  if (T < 1) return 0;
  return (size_t)lmh::row_blocks(T) * (sizeof(double) + sizeof(int64_t));
}

// dna_lm_head_fwd (bias NULL) and dna_lm_head_bias_fwd
static int head_fwd(const char* name, const void* h, int64_t h_stride, int h_dtype, const void* W,
                    int w_dtype, const float* bias, const int64_t* labels, int T, int D, int V,
                    float denom, float* loss_sum, int64_t* count, float* loss, float* coef,
                    void* workspace, size_t workspace_bytes, void* stream) {
  int st = lmh::shape_check(name, T, D, V, h_dtype, w_dtype);
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(h && W && labels && loss_sum && count, "%s: null pointer", name);
  DNA_CHECK_ARG(h_stride >= D, "%s: row stride must be >= D", name);
  const size_t need = dna_lm_head_fwd_workspace(T);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need && aligned(workspace, 8),
                "%s: workspace too small or not 8-byte aligned (%zu < %zu)", name,
                workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int nb = lmh::row_blocks(T);
  const int vec = lmh::pick_vec(h_dtype, D, h, h_stride, W);
  const bool reg = D <= lmh::NCH * 64 * vec;
  double* part_loss = (double*)workspace;
  int64_t* part_cnt = (int64_t*)(part_loss + nb);
  lmh::RowArgs ra{h, h_stride, W, bias, labels, T, D, V, coef, part_loss, part_cnt};
  const dim3 grid((unsigned)nb);
  if (h_dtype == DNA_BF16) {
    if (w_dtype == DNA_BF16) lmh::launch_rows<true, true>(vec, reg, grid, s, ra);
    else lmh::launch_rows<true, false>(vec, reg, grid, s, ra);
  } else {
    if (w_dtype == DNA_BF16) lmh::launch_rows<false, true>(vec, reg, grid, s, ra);
    else lmh::launch_rows<false, false>(vec, reg, grid, s, ra);
  }
  DNA_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(lmh::finish_kernel, dim3(1), dim3(1024), 0, s, (const double*)part_loss,
                     (const int64_t*)part_cnt, nb, denom, loss_sum, count, loss);
  DNA_LAUNCH_CHECK(name);
  return DNA_OK;
}

extern "C" int dna_lm_head_fwd(const void* h, int64_t h_stride, int h_dtype, const void* W,
                               int w_dtype, const int64_t* labels, int T, int D, int V,
                               float denom, float* loss_sum, int64_t* count, float* loss,
                               float* coef, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return head_fwd("dna_lm_head_fwd", h, h_stride, h_dtype, W, w_dtype, nullptr, labels, T, D, V,
                  denom, loss_sum, count, loss, coef, workspace, workspace_bytes, stream);
}

extern "C" int dna_lm_head_bias_fwd(const void* h, int64_t h_stride, int h_dtype, const void* W,
                                    int w_dtype, const float* bias, const int64_t* labels, int T,
                                    int D, int V, float denom, float* loss_sum, int64_t* count,
                                    float* loss, float* coef, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return head_fwd("dna_lm_head_bias_fwd", h, h_stride, h_dtype, W, w_dtype, bias, labels, T, D, V,
                  denom, loss_sum, count, loss, coef, workspace, workspace_bytes, stream);
}

extern "C" size_t dna_lm_head_bwd_workspace(int T, int D, int V) {
  if (T < 1 || D < 1 || V < 1) return 0;
  return (size_t)lmh::dw_nchunks(T) * V * D * sizeof(float);
}

extern "C" size_t dna_lm_head_bias_bwd_workspace(int T, int D, int V) {
  if (T < 1 || D < 1 || V < 1) return 0;
  return dna_lm_head_bwd_workspace(T, D, V) + (size_t)lmh::dw_nchunks(T) * V * sizeof(float);
}

// dna_lm_head_bwd (db NULL) and dna_lm_head_bias_bwd; workspace: dW's partials, then db's
static int head_bwd(const char* name, const float* coef, const void* h, int64_t h_stride,
                    int h_dtype, const void* W, int w_dtype, const int64_t* labels,
                    const int64_t* count, const float* upstream, float denom, int T, int D, int V,
                    void* dh, int64_t dh_stride, float* dW, float* db, int accumulate,
                    void* workspace, size_t workspace_bytes, void* stream) {
  int st = lmh::shape_check(name, T, D, V, h_dtype, w_dtype);
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(coef && W && labels && count, "%s: null pointer", name);
  DNA_CHECK_ARG(!dh || dh_stride >= D, "%s: dh row stride must be >= D", name);
  DNA_CHECK_ARG(!dW || (h && h_stride >= D), "%s: dW needs h with a row stride >= D", name);
  DNA_CHECK_ARG(!db || dW, "%s: dbias is computed with dW only", name);
  DNA_CHECK_ARG((int64_t)V * D <= 0x7fffffff, "%s: V * D too large", name);
  hipStream_t s = as_stream(stream);
  if (dh) {
    lmh::DhArgs da{coef, W, labels, count, upstream, denom, T, D, V, dh, dh_stride};
    const int vec = lmh::pick_vec(h_dtype, D, dh, dh_stride, W);
    const dim3 grid((unsigned)lmh::row_blocks(T));
    if (h_dtype == DNA_BF16) {
      if (w_dtype == DNA_BF16) lmh::launch_dh<true, true>(vec, grid, s, da);
      else lmh::launch_dh<true, false>(vec, grid, s, da);
    } else {
      if (w_dtype == DNA_BF16) lmh::launch_dh<false, true>(vec, grid, s, da);
      else lmh::launch_dh<false, false>(vec, grid, s, da);
    }
    DNA_LAUNCH_CHECK(name);
  }
  if (!dW) return DNA_OK;  // a frozen embedding
  const size_t need = db ? dna_lm_head_bias_bwd_workspace(T, D, V) : dna_lm_head_bwd_workspace(T, D, V);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", name,
                workspace_bytes, need);
  const int nchunks = lmh::dw_nchunks(T);
  float* part = (float*)workspace;
  float* part_b = db ? part + (size_t)nchunks * V * D : nullptr;
  lmh::DwArgs wa{coef, h, h_stride, labels, T, D, V, lmh::dw_chunk_len(T), part, part_b};
  const int ncol = db ? D + 1 : D;
  const dim3 grid((unsigned)((ncol + lmh::TPB - 1) / lmh::TPB), (unsigned)nchunks);
  if (h_dtype == DNA_BF16) lmh::launch_dw<true>(V, grid, s, wa);
  else lmh::launch_dw<false>(V, grid, s, wa);
  DNA_LAUNCH_CHECK(name);
  const int n = V * D;
  hipLaunchKernelGGL(lmh::dw_finish_kernel, dim3((unsigned)((n + lmh::TPB - 1) / lmh::TPB)),
                     dim3(lmh::TPB), 0, s, (const float*)part, nchunks, n, count, upstream, denom,
                     dW, accumulate ? 1 : 0);
  DNA_LAUNCH_CHECK(name);
  if (db) {
    hipLaunchKernelGGL(lmh::dw_finish_kernel, dim3(1), dim3(lmh::TPB), 0, s, (const float*)part_b,
                       nchunks, V, count, upstream, denom, db, accumulate ? 1 : 0);
    DNA_LAUNCH_CHECK(name);
  }
  return DNA_OK;
}

extern "C" int dna_lm_head_bwd(const float* coef, const void* h, int64_t h_stride, int h_dtype,
                               const void* W, int w_dtype, const int64_t* labels,
                               const int64_t* count, const float* upstream, float denom, int T,
                               int D, int V, void* dh, int64_t dh_stride, float* dW,
                               int accumulate, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return head_bwd("dna_lm_head_bwd", coef, h, h_stride, h_dtype, W, w_dtype, labels, count,
                  upstream, denom, T, D, V, dh, dh_stride, dW, nullptr, accumulate, workspace,
                  workspace_bytes, stream);
}

extern "C" int dna_lm_head_bias_bwd(const float* coef, const void* h, int64_t h_stride,
                                    int h_dtype, const void* W, int w_dtype,
                                    const int64_t* labels, const int64_t* count,
                                    const float* upstream, float denom, int T, int D, int V,
                                    void* dh, int64_t dh_stride, float* dW, float* dbias,
                                    int accumulate, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return head_bwd("dna_lm_head_bias_bwd", coef, h, h_stride, h_dtype, W, w_dtype, labels, count,
                  upstream, denom, T, D, V, dh, dh_stride, dW, dbias, accumulate, workspace,
                  workspace_bytes, stream);
}

// ------------------------------------------------------------------------ RC-equivariant head
// workspace of both: Wt [V, 2 D] (4 bytes per element reserved: W is fp32 or bf16) at the base,
// then what the plain entry point takes at width 2 D (backward: dWt [V, 2 D] fp32 before it)
static size_t rc_wt_bytes(int D, int V) { return (size_t)V * 2 * D * sizeof(float); }

static int rc_check(const char* name, int T, int D, int V, int h_dtype, int w_dtype,
                    const void* W, const int64_t* cm, const void* workspace,
                    size_t workspace_bytes, size_t need) {
  int st = lmh::shape_check(name, T, D, V, h_dtype, w_dtype);
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG((int64_t)V * 2 * D <= 0x7fffffff, "%s: V * 2 D too large", name);
  DNA_CHECK_ARG(W && cm, "%s: null pointer", name);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need && aligned(workspace, 16),
                "%s: workspace too small or not 16-byte aligned (%zu < %zu)", name,
                workspace_bytes, need);
  return DNA_OK;
}

static void rc_expand(const void* W, int w_dtype, const int64_t* cm, int D, int V, void* Wt,
                      hipStream_t s) {
  const dim3 grid((unsigned)((V * 2 * D + lmh::TPB - 1) / lmh::TPB));
  if (w_dtype == DNA_BF16)
    hipLaunchKernelGGL(lmh::rc_expand_kernel<true>, grid, dim3(lmh::TPB), 0, s, W, cm, D, V, Wt);
  else
    hipLaunchKernelGGL(lmh::rc_expand_kernel<false>, grid, dim3(lmh::TPB), 0, s, W, cm, D, V, Wt);
}

extern "C" size_t dna_lm_head_rc_fwd_workspace(int T, int D, int V) {
  if (T < 1 || D < 1 || V < 1) return 0;
  return rc_wt_bytes(D, V) + dna_lm_head_fwd_workspace(T);
}

extern "C" int dna_lm_head_rc_fwd(const void* h, int64_t h_stride, int h_dtype, const void* W,
                                  int w_dtype, const int64_t* cm, const int64_t* labels, int T,
                                  int D, int V, float denom, float* loss_sum, int64_t* count,
                                  float* loss, float* coef, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  int st = rc_check("dna_lm_head_rc_fwd", T, D, V, h_dtype, w_dtype, W, cm, workspace,
                    workspace_bytes, dna_lm_head_rc_fwd_workspace(T, D, V));
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(h && labels && loss_sum && count, "dna_lm_head_rc_fwd: null pointer");
  DNA_CHECK_ARG(h_stride >= 2 * (int64_t)D, "dna_lm_head_rc_fwd: row stride must be >= 2 D");
  rc_expand(W, w_dtype, cm, D, V, workspace, as_stream(stream));
  DNA_LAUNCH_CHECK("dna_lm_head_rc_fwd");
  const size_t off = rc_wt_bytes(D, V);
  return dna_lm_head_fwd(h, h_stride, h_dtype, workspace, w_dtype, labels, T, 2 * D, V, denom,
                         loss_sum, count, loss, coef, (char*)workspace + off,
                         workspace_bytes - off, stream);
}

extern "C" size_t dna_lm_head_rc_bwd_workspace(int T, int D, int V) {
  if (T < 1 || D < 1 || V < 1) return 0;
  return 2 * rc_wt_bytes(D, V) + dna_lm_head_bwd_workspace(T, 2 * D, V);
}

extern "C" int dna_lm_head_rc_bwd(const float* coef, const void* h, int64_t h_stride, int h_dtype,
                                  const void* W, int w_dtype, const int64_t* cm,
                                  const int64_t* labels, const int64_t* count,
                                  const float* upstream, float denom, int T, int D, int V,
                                  void* dh, int64_t dh_stride, float* dW, int accumulate,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  int st = rc_check("dna_lm_head_rc_bwd", T, D, V, h_dtype, w_dtype, W, cm, workspace,
                    workspace_bytes, dna_lm_head_rc_bwd_workspace(T, D, V));
  if (st != DNA_OK) return st;
  DNA_CHECK_ARG(coef && labels && count, "dna_lm_head_rc_bwd: null pointer");
  DNA_CHECK_ARG(!dh || dh_stride >= 2 * (int64_t)D,
                "dna_lm_head_rc_bwd: dh row stride must be >= 2 D");
  DNA_CHECK_ARG(!dW || (h && h_stride >= 2 * (int64_t)D),
                "dna_lm_head_rc_bwd: dW needs h with a row stride >= 2 D");
  hipStream_t s = as_stream(stream);
  if (dh) {  // the only reader of Wt in the backward
    rc_expand(W, w_dtype, cm, D, V, workspace, s);
    DNA_LAUNCH_CHECK("dna_lm_head_rc_bwd");
  }
  const size_t off = rc_wt_bytes(D, V);
  float* dWt = dW ? (float*)((char*)workspace + off) : nullptr;
  st = dna_lm_head_bwd(coef, h, h_stride, h_dtype, workspace, w_dtype, labels, count, upstream,
                       denom, T, 2 * D, V, dh, dh_stride, dWt, 0, (char*)workspace + 2 * off,
                       workspace_bytes - 2 * off, stream);
  if (st != DNA_OK || !dW) return st;
  hipLaunchKernelGGL(lmh::rc_fold_kernel, dim3((unsigned)((V * D + lmh::TPB - 1) / lmh::TPB)),
                     dim3(lmh::TPB), 0, s, (const float*)dWt, cm, D, V, dW, accumulate ? 1 : 0);
  DNA_LAUNCH_CHECK("dna_lm_head_rc_bwd");
  return DNA_OK;
}
