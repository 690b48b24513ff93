// Batch assembly from a device-resident split of character-tokenised sequences (resident.py).
//
// The split keeps every sequence's bytes concatenated in `bases` (offsets [N + 1]), a 256-entry
// byte -> output-id table and a 256-entry complement table. dna_char_batch builds one batch in one
// launch: row r takes sequence s = idx[r] of n = offsets[s + 1] - offsets[s] bytes and writes
//
//   keep = min(n, L - eos)                                  (eos = 1 when eos_id >= 0)
//   token j < keep     lut[bases[off + j]]                  or, with rc[r] set,
//                      lut[comp[bases[off + n - 1 - j]]]    (reverse complement, then truncate)
//   token keep         eos_id, when there is one
//   L - keep - eos     pad_id cells, on the left (pad_left) or the right
//
// and, on request, the mask (0 exactly on the pad cells). A plain gather: one workgroup per row,
// lanes over positions, so the byte loads and the 8-byte id stores of a wave are contiguous. The
// two tables sit in LDS, already composed for the reverse strand. Nothing outside
// bases[off .. off + n) is read: a row whose idx or offsets are out of range (the host checks
// them before it uploads an epoch) is written as all padding.
#include "common.h"

namespace dna {
namespace cbatch {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void char_batch_kernel(
    const uint8_t* __restrict__ bases, int64_t n_bases, const int64_t* __restrict__ offsets,
    int64_t n_seqs, const int64_t* __restrict__ idx, const uint8_t* __restrict__ rc,
    const int64_t* __restrict__ lut, const uint8_t* __restrict__ comp, int L, int pad_left,
    int64_t pad_id, int64_t eos_id, int64_t* __restrict__ ids, uint8_t* __restrict__ mask) {
  __shared__ int64_t fwd[256], rev[256];
  fwd[threadIdx.x] = lut[threadIdx.x];
  rev[threadIdx.x] = lut[comp[threadIdx.x]];
  __syncthreads();
  const int r = blockIdx.x;
  const int64_t s = idx[r];
  int64_t off = 0, n = 0;
  if (s >= 0 && s < n_seqs) {
    off = offsets[s];
    n = offsets[s + 1] - off;
    if (off < 0 || n < 0 || off + n > n_bases) n = 0;
  }
  const bool flip = rc != nullptr && rc[r] != 0;
  const int eos = eos_id >= 0 ? 1 : 0;
  const int keep = (int)(n < (int64_t)(L - eos) ? n : (int64_t)(L - eos));
  const int first = pad_left ? L - keep - eos : 0;  // the position of token 0
  int64_t* out = ids + (size_t)r * L;
  uint8_t* mout = mask ? mask + (size_t)r * L : nullptr;
  for (int p = threadIdx.x; p < L; p += THREADS) {
    const int t = p - first;
    int64_t v = pad_id;
    uint8_t m = 0;
    if (t >= 0 && t < keep) {
      v = flip ? rev[bases[off + (n - 1 - t)]] : fwd[bases[off + t]];
      m = 1;
    } else if (eos && t == keep) {
      v = eos_id;
      m = 1;
    }
    out[p] = v;
    if (mout) mout[p] = m;
  }
}

}  // namespace cbatch
}  // namespace dna

using namespace dna;

extern "C" int dna_char_batch(const uint8_t* bases, int64_t n_bases, const int64_t* offsets,
                              int64_t n_seqs, const int64_t* idx, const uint8_t* rc,
                              const int64_t* lut, const uint8_t* comp, int B, int L, int pad_left,
                              int64_t pad_id, int64_t eos_id, int64_t* ids, uint8_t* mask,
                              void* stream) {
  DNA_CHECK_ARG(bases && offsets && idx && lut && comp && ids, "dna_char_batch: null pointer");
  DNA_CHECK_ARG(n_bases >= 0 && n_seqs >= 1, "dna_char_batch: bad split (n_bases %lld, n_seqs %lld)",
                (long long)n_bases, (long long)n_seqs);
  DNA_CHECK_ARG(B >= 0 && L >= 1, "dna_char_batch: bad batch (B %d, L %d)", B, L);
  DNA_CHECK_ARG(pad_id >= 0, "dna_char_batch: pad_id %lld < 0", (long long)pad_id);
  DNA_CHECK_ARG(aligned(offsets, 8) && aligned(idx, 8) && aligned(lut, 8) && aligned(ids, 8),
                "dna_char_batch: offsets, idx, lut and ids must be 8-B aligned");
  if (B == 0) return DNA_OK;
  hipLaunchKernelGGL(cbatch::char_batch_kernel, dim3(B), dim3(cbatch::THREADS), 0,
                     as_stream(stream), bases, n_bases, offsets, n_seqs, idx, rc, lut, comp, L,
                     pad_left, pad_id, eos_id, ids, mask);
  DNA_LAUNCH_CHECK("dna_char_batch");
  return DNA_OK;
}
