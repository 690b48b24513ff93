// Batch assembly from a device-resident genome (genome.py, resident.ResidentWindows).
//
// A genome store keeps its records (chromosomes) concatenated in `bases`, one byte per base, and
// a 256-entry byte -> output-id table. The host decides every row -- where its window starts
// (src, an absolute offset into `bases`), how many bases it reads (n) and how many fill cells
// stand in front of them (left) -- and dna_genome_windows builds the batch in one launch. Row r,
// cut at L cells, is
//
//   fill_id x left[r] | lut[bases[src[r] + j]], j = 0 .. n[r] - 1 | eos_id (if >= 0) | fill_id ...
//
// A plain gather like char_batch.hip, but parallel over (row, chunk of CHUNK positions): a
// species batch is 1-8 rows of up to 131,072 cells, so one row alone spreads over L / CHUNK
// workgroups. Within a chunk the lanes run over consecutive positions, so a wave's byte loads
// and 8-byte id stores are contiguous (src is not aligned: byte loads, no head / tail path). The
// table sits in LDS. Every cell of ids is written exactly once. All offsets are 64-bit (a genome
// is larger than 2^31 bytes). Nothing outside bases[src .. src + n) is read: a row with src < 0,
// n < 0, left < 0 or src + n > n_bases (the host checks them before it uploads a pass) is
// written as all fill_id.
#include "common.h"

namespace dna {
namespace gwin {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;
constexpr int CHUNK = THREADS * PER_THREAD;  // positions of one workgroup

__global__ __launch_bounds__(THREADS) void genome_windows_kernel(
    const uint8_t* __restrict__ bases, int64_t n_bases, const int64_t* __restrict__ src,
    const int32_t* __restrict__ n, const int32_t* __restrict__ left,
    const int64_t* __restrict__ lut, int L, int chunks, int64_t fill_id, int64_t eos_id,
    int64_t* __restrict__ ids) {
  __shared__ int64_t tab[256];
  tab[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int r = blockIdx.x / chunks;
  const int p0 = (blockIdx.x - r * chunks) * CHUNK;
  int64_t off = src[r];
  int nr = n[r], lf = left[r];
  if (off < 0 || nr < 0 || lf < 0 || off > n_bases - (int64_t)nr) {  // invalid: all fill
    off = 0;
    nr = 0;
    lf = L;
  }
  const uint8_t* row = bases + off;
  int64_t* out = ids + (int64_t)r * L;
#pragma unroll
  for (int i = 0; i < PER_THREAD; ++i) {
    const int p = p0 + i * THREADS + (int)threadIdx.x;
    if (p >= L) break;
    // p < L and 0 <= lf: p - lf cannot overflow; t < nr keeps the load inside [src, src + n)
    const int t = p - lf;
    int64_t v = fill_id;
    if (t >= 0 && t < nr)
      v = tab[row[t]];
    else if (t == nr && eos_id >= 0)
      v = eos_id;
    out[p] = v;
  }
}

}  // namespace gwin
}  // namespace dna

using namespace dna;

extern "C" int dna_genome_windows(const uint8_t* bases, int64_t n_bases, const int64_t* src,
                                  const int32_t* n, const int32_t* left, const int64_t* lut, int B,
                                  int L, int64_t fill_id, int64_t eos_id, int64_t* ids,
                                  void* stream) {
  DNA_CHECK_ARG(bases && src && n && left && lut && ids, "dna_genome_windows: null pointer");
  DNA_CHECK_ARG(n_bases >= 0, "dna_genome_windows: n_bases %lld < 0", (long long)n_bases);
  DNA_CHECK_ARG(B >= 0 && L >= 1, "dna_genome_windows: bad batch (B %d, L %d)", B, L);
  DNA_CHECK_ARG(fill_id >= 0, "dna_genome_windows: fill_id %lld < 0", (long long)fill_id);
  DNA_CHECK_ARG(aligned(src, 8) && aligned(lut, 8) && aligned(ids, 8) && aligned(n, 4) &&
                    aligned(left, 4),
                "dna_genome_windows: src, lut and ids must be 8-B aligned, n and left 4-B");
  if (B == 0) return DNA_OK;
  const int chunks = (L + gwin::CHUNK - 1) / gwin::CHUNK;
  DNA_CHECK_ARG((int64_t)B * chunks <= 0x7fffffffLL,
                "dna_genome_windows: B %d x %d chunks exceeds the grid", B, chunks);
  hipLaunchKernelGGL(gwin::genome_windows_kernel, dim3((unsigned)(B * chunks)),
                     dim3(gwin::THREADS), 0, as_stream(stream), bases, n_bases, src, n, left, lut,
                     L, chunks, fill_id, eos_id, ids);
  DNA_LAUNCH_CHECK("dna_genome_windows");
  return DNA_OK;
}
