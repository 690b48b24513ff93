// Sequence-classification head of DNABERT-2 (reference bert_layers.py:495-510 BertPooler,
// :881-1009 BertForSequenceClassification): pooler, dropout, classifier and loss, forward and
// backward, on the fp32 master weights (no bf16 shadow, no transposed copy).
//
//   t = tanh(x Wp^T + bp)      a = dropout(t)      logits = a Wc^T + bc      loss(logits, labels)
//
// x is B rows of H (fp32 or bf16) with a row stride in elements, so the [CLS] rows are read in
// place. Everything is plain fp32 VALU FMA: the head is latency-bound (2 B H^2 FLOP, 0.04 GFLOP at
// B = 32), the operands are read once from L2, and the summation orders below are fixed, so the
// results are bit-identical from run to run. No atomics, no hand-off between workgroups inside a
// launch: the classifier's reduction over H is split over the column tiles of the pooler kernel,
// which write partial logits to a workspace; the next launch sums them in tile order.
//
// Launches: forward 2 (pool_kernel, finish_loss_kernel -- the loss rides in the second when labels
// are given), backward 2 (dz_kernel, then one tn_kernel launch for dWp/dbp, dx and dWc/dbc).
#include <math.h>

#include <type_traits>

#include "cls_loss.h"
#include "common.h"

namespace dna {
namespace cls {

constexpr int RT = 8;      // batch rows per workgroup of the pooler kernel
constexpr int CT_MAX = 64;  // pooler output columns per workgroup: 16 or 64

// four consecutive elements idx .. idx + 3 of an fp32 or bf16 array, as fp32. The dtype is a
// template parameter: a run-time branch around every load makes the compiler wait for each load
// before it issues the next
template <bool BF>
__device__ __forceinline__ float4 ld4(const void* p, size_t idx) {
  if constexpr (BF) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(p) + idx);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  } else {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + idx);
  }
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

// ------------------------------------------------------------------------------ forward: pooler
struct PoolArgs {
  const void* x; int x_bf16; long row_stride;
  const float* Wp; const float* bp; const float* Wc;
  int B, H, C, ct;
  float p; uint32_t th; float ks; uint64_t seed, off;
  float* t; float* a; float* part;  // part [H / ct][B][C]
};

// One workgroup: RT batch rows x ct output columns. A wave owns ct / 4 columns and takes them
// four at a time; its lanes split the reduction over H (16-B loads, a Wp row is read as
// contiguous 1-KiB pieces), so each lane holds 4 x RT partial sums. They are summed over the 64
// lanes by a halving exchange: each step sends half of a lane's values to its partner and keeps
// the other half (32 -> 16 -> 8 -> 4 -> 2 -> 1 values, lane bits 5 .. 1), then one last exchange
// over bit 0: 32 shuffles for 32 sums, and the order of the additions is fixed.
// KS > 0: H <= 256 KS, the x rows stay in registers; KS = 0: any H, x is re-read per column group.
template <int KS, bool BF>
__global__ __launch_bounds__(256) void pool_kernel(PoolArgs g) {
  __shared__ float a_tile[RT][CT_MAX + 1];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.y * RT, j0 = blockIdx.x * g.ct;
  const int cpw = g.ct >> 2;
  const int H = g.H, B = g.B;
  size_t xrow[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) xrow[r] = (size_t)min(b0 + r, B - 1) * g.row_stride;

  float4 xr[RT][KS > 0 ? KS : 1];
  if constexpr (KS > 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = s * 256 + lane * 4;
        xr[r][s] = k < H ? ld4<BF>(g.x, xrow[r] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }

  for (int cb = 0; cb < cpw; cb += 4) {
    const int jb = j0 + w * cpw + cb;  // first of this wave's four columns (a multiple of 4)
    float v[4 * RT];
#pragma unroll
    for (int i = 0; i < 4 * RT; ++i) v[i] = 0.f;
    if constexpr (KS > 0) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = s * 256 + lane * 4;
        if (k < H) {
          float4 wv[4];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            wv[c] = *reinterpret_cast<const float4*>(g.Wp + (size_t)(jb + c) * H + k);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < RT; ++r) v[c * RT + r] = dot4(wv[c], xr[r][s], v[c * RT + r]);
        }
      }
    } else {
      for (int k = lane * 4; k < H; k += 256) {
        float4 wv[4], xv[RT];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          wv[c] = *reinterpret_cast<const float4*>(g.Wp + (size_t)(jb + c) * H + k);
#pragma unroll
        for (int r = 0; r < RT; ++r) xv[r] = ld4<BF>(g.x, xrow[r] + k);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < RT; ++r) v[c * RT + r] = dot4(wv[c], xv[r], v[c * RT + r]);
      }
    }
    // halving exchange: afterwards the lane holds the sum of value (lane >> 1)
#pragma unroll
    for (int n = 4 * RT, m = 32; n > 1; n >>= 1, m >>= 1) {
      const bool upper = (lane & m) != 0;
#pragma unroll
      for (int i = 0; i < n / 2; ++i) {
        // values first, then the selects: `upper ? v[i] : v[j]` on the array elements themselves
        // is a select of addresses, which puts v[] in dynamically indexed storage
        const float lo = v[i], hi = v[i + n / 2];
        const float send = upper ? lo : hi;
        const float keep = upper ? hi : lo;
        v[i] = keep + __shfl_xor(send, m, 64);
      }
    }
    float z = v[0] + __shfl_xor(v[0], 1, 64);
    const int c = lane >> 4, r = (lane >> 1) & 7;  // value index (lane >> 1) = c * RT + r
    const int j = jb + c, b = b0 + r;
    z += g.bp[j];
    const float tv = tanhf(z);
    float av = tv;
    if (g.p > 0.f) {
      const uint64_t e = (uint64_t)min(b, B - 1) * H + j;
      const bool kept = (dropout_keep4(g.seed, g.off, e >> 2, g.th) >> (e & 3)) & 1;
      av = kept ? tv * g.ks : 0.f;
    }
    if ((lane & 1) == 0) {
      a_tile[r][j - j0] = av;
      if (b < B) {
        g.t[(size_t)b * H + j] = tv;
        g.a[(size_t)b * H + j] = av;
      }
    }
  }
  __syncthreads();
  // this column tile's share of the logits: part[tile][b][c] = sum_j a[b][j] Wc[c][j]
  for (int o = threadIdx.x; o < RT * g.C; o += 256) {
    const int r = o / g.C, c = o - r * g.C;
    if (b0 + r >= B) continue;
    // the ct <= 64 classifier weights as 16-B loads, all in flight before the first FMA
    const float4* wc = reinterpret_cast<const float4*>(g.Wc + (size_t)c * H + j0);
    float4 wv[CT_MAX / 4];
#pragma unroll
    for (int q = 0; q < CT_MAX / 4; ++q)
      wv[q] = q * 4 < g.ct ? wc[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < CT_MAX / 4; ++q) {
      if (q * 4 < g.ct) {
        s = fmaf(a_tile[r][q * 4 + 0], wv[q].x, s);
        s = fmaf(a_tile[r][q * 4 + 1], wv[q].y, s);
        s = fmaf(a_tile[r][q * 4 + 2], wv[q].z, s);
        s = fmaf(a_tile[r][q * 4 + 3], wv[q].w, s);
      }
    }
    g.part[((size_t)blockIdx.x * B + b0 + r) * g.C + c] = s;
  }
}

// ------------------------------------------------------------ forward: logits from partials, loss
struct LossArgs {
  const float* part; int nparts; const float* bc;  // part != NULL: logits = bc + sum of partials
  float* logits;                                   // written (part != NULL) or read
  const void* labels; int problem;                 // labels NULL: no loss
  int B, C;
  float* loss; float* dlogits; int64_t* pred;
};

// One workgroup: first the logits (an element per thread), then, behind a workgroup barrier, the
// loss with a thread per row and the row arithmetic in float (cls_loss.h).
__global__ __launch_bounds__(1024) void finish_loss_kernel(LossArgs g) {
  const int tid = threadIdx.x, B = g.B, C = g.C;
  if (g.part) {
    // logits = bc + the column tiles' partial sums, in tile order; one element per thread and
    // pass, the loads of a group of tiles in flight together
    const size_t n = (size_t)B * C;
    for (size_t e = tid; e < n; e += 1024) {
      float v = g.bc[e % C];
#pragma unroll 8
      for (int q = 0; q < g.nparts; ++q) v += g.part[(size_t)q * n + e];
      g.logits[e] = v;
    }
    if (!g.labels) return;
    __syncthreads();  // the rows below are read by other threads of this workgroup
  }
  cls_loss<float>(g.logits, g.labels, g.problem, B, C, g.loss, g.dlogits, g.pred);
}

// ------------------------------------------------------------------------------------ backward
struct DzArgs {
  const float* dl; const float* upstream; const float* t; const float* Wc;
  int B, H, C;
  float p; uint32_t th; float ks; uint64_t seed, off;
  float* dz;
};

// dz = (dlogits Wc) * keep / (1 - p) * (1 - t^2), four columns per thread; the keep bits come
// from the same (seed, offset, element) draws as the forward's
__global__ __launch_bounds__(256) void dz_kernel(DzArgs g) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int H4 = g.H >> 2;
  if (idx >= (size_t)g.B * H4) return;
  const int b = (int)(idx / H4), h = (int)(idx - (size_t)b * H4) * 4;
  float4 da = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < g.C; ++c) {
    const float d = g.dl[(size_t)b * g.C + c];
    const float4 w = *reinterpret_cast<const float4*>(g.Wc + (size_t)c * g.H + h);
    da.x = fmaf(d, w.x, da.x);
    da.y = fmaf(d, w.y, da.y);
    da.z = fmaf(d, w.z, da.z);
    da.w = fmaf(d, w.w, da.w);
  }
  const float up = g.upstream ? g.upstream[0] : 1.f;
  const size_t e = (size_t)b * g.H + h;
  const uint32_t m = g.p > 0.f ? dropout_keep4(g.seed, g.off, e >> 2, g.th) : 0xFu;
  const float4 tv = *reinterpret_cast<const float4*>(g.t + e);
  float4 o;
  o.x = da.x * up * ((m & 1u) ? g.ks : 0.f) * (1.f - tv.x * tv.x);
  o.y = da.y * up * ((m & 2u) ? g.ks : 0.f) * (1.f - tv.y * tv.y);
  o.z = da.z * up * ((m & 4u) ? g.ks : 0.f) * (1.f - tv.z * tv.z);
  o.w = da.w * up * ((m & 8u) ? g.ks : 0.f) * (1.f - tv.w * tv.w);
  *reinterpret_cast<float4*>(g.dz + e) = o;
}

// out[i][j] (+)= scale * sum_r L(r, i) R(r, j), lsum[i] (+)= scale * sum_r L(r, i)
//   L(r, i) = L[r * l_red + i * l_i]  (fp32),  R(r, j) = R[r * ldr + j]  (fp32 or bf16)
// covers the three products of the backward:
//   dWp = dz^T x   (+ dbp)      dx = dz Wp      dWc = dlogits^T a   (+ dbc)
struct Prob {
  const float* L; long l_red, l_i;
  const void* R; int r_bf16; long ldr;
  int M, N, K;
  float* out; int accumulate; const float* scale;
  float* lsum;
  int tiles_j, blocks;
};
struct TnArgs { Prob p[3]; };

constexpr int NW = 16;  // waves per workgroup = slices of the reduction

// One workgroup: IT rows x 256 columns of one product. Wave w sums r = w, w + NW, ...; a lane
// holds four columns (one 16-B load of R per r), the IT values of L are the same for the whole
// wave. The NW slices are then added in slice order through LDS, two rows of the tile at a time.
template <int IT, bool BF>
__device__ __forceinline__ void tn_accumulate(const Prob& P, int w, int j, bool jok,
                                              const size_t (&loff)[IT], float4 (&acc)[IT],
                                              float (&ls)[IT]) {
#pragma unroll(IT > 8 ? 2 : 4)
  for (int r = w; r < P.K; r += NW) {
    const float4 rv = jok ? ld4<BF>(P.R, (size_t)r * P.ldr + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float* lrow = P.L + (size_t)r * P.l_red;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const float li = lrow[loff[i]];
      acc[i].x = fmaf(li, rv.x, acc[i].x);
      acc[i].y = fmaf(li, rv.y, acc[i].y);
      acc[i].z = fmaf(li, rv.z, acc[i].z);
      acc[i].w = fmaf(li, rv.w, acc[i].w);
      ls[i] += li;
    }
  }
}

template <int IT>
__global__ __launch_bounds__(1024) void tn_kernel(TnArgs g) {
  __shared__ float red[NW][2][256];
  __shared__ float lred[NW][IT];
  int bid = blockIdx.x, q = 0;
  while (q < 2 && bid >= g.p[q].blocks) {
    bid -= g.p[q].blocks;
    ++q;
  }
  const Prob P = q == 0 ? g.p[0] : q == 1 ? g.p[1] : g.p[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i0 = (bid / P.tiles_j) * IT, jt = bid % P.tiles_j;
  const int j = jt * 256 + lane * 4;
  const bool jok = j < P.N;
  float4 acc[IT];
  float ls[IT];
  size_t loff[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    ls[i] = 0.f;
    loff[i] = (size_t)min(i0 + i, P.M - 1) * P.l_i;  // rows past M: a valid address, never stored
  }
  if (P.r_bf16)  // wave-uniform, once around the whole loop
    tn_accumulate<IT, true>(P, w, j, jok, loff, acc, ls);
  else
    tn_accumulate<IT, false>(P, w, j, jok, loff, acc, ls);
  const float scale = P.scale ? P.scale[0] : 1.f;
#pragma unroll
  for (int i = 0; i < IT; i += 2) {
    *reinterpret_cast<float4*>(&red[w][0][lane * 4]) = acc[i];
    *reinterpret_cast<float4*>(&red[w][1][lane * 4]) = acc[i + 1];
    __syncthreads();
    if (tid < 512) {
      const int h = tid >> 8, jj = tid & 255;
      float s = red[0][h][jj];
#pragma unroll
      for (int u = 1; u < NW; ++u) s += red[u][h][jj];
      const int row = i0 + i + h, col = jt * 256 + jj;
      if (row < P.M && col < P.N) {
        float* o = P.out + (size_t)row * P.N + col;
        *o = P.accumulate ? *o + s * scale : s * scale;
      }
    }
    __syncthreads();
  }
  if (P.lsum && jt == 0) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < IT; ++i) lred[w][i] = ls[i];
    }
    __syncthreads();
    if (tid < IT && i0 + tid < P.M) {
      float s = lred[0][tid];
#pragma unroll
      for (int u = 1; u < NW; ++u) s += lred[u][tid];
      float* o = P.lsum + i0 + tid;
      *o = P.accumulate ? *o + s * scale : s * scale;
    }
  }
}

template <int IT>
static Prob make_prob(const float* L, long l_red, long l_i, const void* R, int r_bf16, long ldr,
                      int M, int N, int K, float* out, int accumulate, const float* scale,
                      float* lsum) {
  Prob p{L, l_red, l_i, R, r_bf16, ldr, M, N, K, out, accumulate, scale, lsum, 0, 0};
  p.tiles_j = (N + 255) / 256;
  p.blocks = ((M + IT - 1) / IT) * p.tiles_j;
  return p;
}

static int pool_ct(int B) { return ((B + RT - 1) / RT) * 4 >= 64 ? 64 : 16; }

}  // namespace cls
}  // namespace dna

using namespace dna;

#define DNA_CLS_SHAPE_CHECK(name)                                                              \
  DNA_CHECK_ARG(B >= 1 && B <= DNA_CLS_MAX_BATCH, name ": batch must be in [1, %d] (got %d)",   \
                DNA_CLS_MAX_BATCH, B);                                                         \
  DNA_CHECK_ARG(H >= 64 && H % 64 == 0, name ": hidden size must be a multiple of 64 (got %d)", H); \
  DNA_CHECK_ARG(C >= 1 && C <= 64, name ": 1 <= labels <= 64 required (got %d)", C);           \
  DNA_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, name ": dropout p must be in [0, 1)");          \
  DNA_CHECK_ARG(x_dtype == DNA_F32 || x_dtype == DNA_BF16, name ": x must be fp32 or bf16");   \
  DNA_CHECK_ARG(x_row_stride >= H && x_row_stride % 4 == 0,                                    \
                name ": x row stride must be >= H and a multiple of 4 (got %ld)", (long)x_row_stride); \
  DNA_CHECK_ARG(aligned(x, x_dtype == DNA_BF16 ? 8 : 16), name ": x must be 16-byte aligned")

extern "C" size_t dna_cls_head_fwd_workspace(int B, int H, int C) {
  if (B < 1 || H < 64 || C < 1) return 0;
  return (size_t)(H / cls::pool_ct(B)) * B * C * sizeof(float);
}

static int cls_loss_check(const char* name, int problem, const void* labels, const float* loss,
                          const float* dlogits) {
  DNA_CHECK_ARG(problem == DNA_CLS_REGRESSION || problem == DNA_CLS_SINGLE_LABEL ||
                    problem == DNA_CLS_MULTI_LABEL,
                "%s: bad problem type %d", name, problem);
  DNA_CHECK_ARG(labels && loss && dlogits, "%s: null labels / loss / dlogits", name);
  return DNA_OK;
}

extern "C" int dna_cls_head_fwd(const void* x, int x_dtype, int64_t x_row_stride, const float* Wp,
                                const float* bp, const float* Wc, const float* bc, int B, int H,
                                int C, float p_drop, uint64_t seed, uint64_t offset, float* t,
                                float* a, float* logits, const void* labels, int problem_type,
                                float* loss, float* dlogits, int64_t* pred, void* workspace,
                                size_t workspace_bytes, void* stream) {
  DNA_CHECK_ARG(x && Wp && bp && Wc && bc && t && a && logits, "dna_cls_head_fwd: null pointer");
  DNA_CLS_SHAPE_CHECK("dna_cls_head_fwd");
  DNA_CHECK_ARG(aligned(Wp, 16) && aligned(Wc, 16) && aligned(t, 16) &&
                    aligned(a, 16),
                "dna_cls_head_fwd: Wp / Wc / t / a must be 16-byte aligned");
  if (labels) {
    int st = cls_loss_check("dna_cls_head_fwd", problem_type, labels, loss, dlogits);
    if (st != DNA_OK) return st;
  }
  const size_t need = dna_cls_head_fwd_workspace(B, H, C);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need,
                "dna_cls_head_fwd: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  const int ct = cls::pool_ct(B);
  cls::PoolArgs pa{x, x_dtype == DNA_BF16, (long)x_row_stride, Wp, bp, Wc, B, H, C, ct, p_drop,
                   dropout_threshold(p_drop), 1.f / (1.f - p_drop), seed, offset, t, a,
                   (float*)workspace};
  dim3 grid(H / ct, (B + cls::RT - 1) / cls::RT);
  auto launch = [&](auto bf) {
    constexpr bool BF = decltype(bf)::value;
    switch (H <= 1024 ? (H + 255) / 256 : 0) {
      case 1: hipLaunchKernelGGL((cls::pool_kernel<1, BF>), grid, dim3(256), 0, s, pa); break;
      case 2: hipLaunchKernelGGL((cls::pool_kernel<2, BF>), grid, dim3(256), 0, s, pa); break;
      case 3: hipLaunchKernelGGL((cls::pool_kernel<3, BF>), grid, dim3(256), 0, s, pa); break;
      case 4: hipLaunchKernelGGL((cls::pool_kernel<4, BF>), grid, dim3(256), 0, s, pa); break;
      default: hipLaunchKernelGGL((cls::pool_kernel<0, BF>), grid, dim3(256), 0, s, pa); break;
    }
  };
  if (x_dtype == DNA_BF16)
    launch(std::true_type{});
  else
    launch(std::false_type{});
  DNA_LAUNCH_CHECK("dna_cls_head_fwd");
  cls::LossArgs la{(const float*)workspace, H / ct, bc, logits, labels, problem_type, B, C, loss,
                   dlogits, pred};
  hipLaunchKernelGGL(cls::finish_loss_kernel, dim3(1), dim3(1024), 0, s, la);
  DNA_LAUNCH_CHECK("dna_cls_head_fwd");
  return DNA_OK;
}

extern "C" int dna_cls_loss(const float* logits, const void* labels, int problem_type, int B, int C,
                            float* loss, float* dlogits, int64_t* pred, void* stream) {
  DNA_CHECK_ARG(logits, "dna_cls_loss: null logits");
  DNA_CHECK_ARG(B >= 1, "dna_cls_loss: batch must be >= 1 (got %d)", B);
  DNA_CHECK_ARG(C >= 1 && C <= 64, "dna_cls_loss: 1 <= labels <= 64 required (got %d)", C);
  int st = cls_loss_check("dna_cls_loss", problem_type, labels, loss, dlogits);
  if (st != DNA_OK) return st;
  cls::LossArgs la{nullptr, 0, nullptr, const_cast<float*>(logits), labels, problem_type, B, C,
                   loss, dlogits, pred};
  hipLaunchKernelGGL(cls::finish_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), la);
  DNA_LAUNCH_CHECK("dna_cls_loss");
  return DNA_OK;
}

extern "C" size_t dna_cls_head_bwd_workspace(int B, int H, int C) {
  (void)C;
  if (B < 1 || H < 64) return 0;
  return (size_t)B * H * sizeof(float);
}

extern "C" int dna_cls_head_bwd(const float* dlogits, const float* upstream, const void* x,
                                int x_dtype, int64_t x_row_stride, const float* t, const float* a,
                                const float* Wp, const float* Wc, int B, int H, int C, float p_drop,
                                uint64_t seed, uint64_t offset, float* dWc, float* dbc, float* dWp,
                                float* dbp, float* dx, int accumulate, void* workspace,
                                size_t workspace_bytes, void* stream) {
  DNA_CHECK_ARG(dlogits && x && t && a && Wp && Wc && dWc && dbc && dWp && dbp && dx,
                "dna_cls_head_bwd: null pointer");
  DNA_CLS_SHAPE_CHECK("dna_cls_head_bwd");
  DNA_CHECK_ARG(aligned(Wp, 16) && aligned(Wc, 16) && aligned(t, 16) &&
                    aligned(a, 16) && aligned(workspace, 16),
                "dna_cls_head_bwd: Wp / Wc / t / a / workspace must be 16-byte aligned");
  const size_t need = dna_cls_head_bwd_workspace(B, H, C);
  DNA_CHECK_ARG(workspace && workspace_bytes >= need,
                "dna_cls_head_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  float* dz = (float*)workspace;
  cls::DzArgs da{dlogits, upstream, t, Wc, B, H, C, p_drop, dropout_threshold(p_drop),
                 1.f / (1.f - p_drop), seed, offset, dz};
  const size_t n4 = (size_t)B * (H / 4);
  hipLaunchKernelGGL(cls::dz_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, da);
  DNA_LAUNCH_CHECK("dna_cls_head_bwd");
  const int acc = accumulate ? 1 : 0;
  const int xb = x_dtype == DNA_BF16;
  auto launch = [&](auto it) {
    constexpr int IT = decltype(it)::value;
    cls::TnArgs ta;
    ta.p[0] = cls::make_prob<IT>(dz, H, 1, x, xb, (long)x_row_stride, H, H, B, dWp, acc, nullptr, dbp);
    ta.p[1] = cls::make_prob<IT>(dz, 1, H, Wp, 0, H, B, H, H, dx, 0, nullptr, nullptr);
    ta.p[2] = cls::make_prob<IT>(dlogits, C, 1, a, 0, H, C, H, B, dWc, acc, upstream, dbc);
    const int blocks = ta.p[0].blocks + ta.p[1].blocks + ta.p[2].blocks;
    hipLaunchKernelGGL(cls::tn_kernel<IT>, dim3(blocks), dim3(1024), 0, s, ta);
  };
  if (B >= 128)
    launch(std::integral_constant<int, 16>{});
  else
    launch(std::integral_constant<int, 8>{});
  DNA_LAUNCH_CHECK("dna_cls_head_bwd");
  return DNA_OK;
}
