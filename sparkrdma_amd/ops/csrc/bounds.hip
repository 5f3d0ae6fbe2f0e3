// Range partitioning by arbitrary split points for MI355X (gfx950): the
// splitter search fused into the wide-record pair extraction.
//
// A RangePartitioner built from real split points (sampled TeraSort
// bounds, non-pow2 key spans) has no closed-form partition function, so it
// cannot be a PartFunc of kernels.hip's digit_of. The search runs ONCE per
// record, here, and writes the partition id into pair.x; everything after
// it (hist, scatter, gather) sees a plain `func 0, shift 0` digit — the
// route the >4096-partition path already takes. The hot kernels of
// kernels.hip are not touched and live in another translation unit.
//
//   pid(key) = #{ i : bounds[i] <= key }, unsigned 64-bit compare
//            = numpy.searchsorted(bounds, key, side="right")
//
// nbounds <= 4095: the block stages the whole table in LDS once (at most
//   32 KB, so four blocks per CU fit the 160 KiB) and every record runs a
//   branch-free binary search of ceil(log2 R) LDS probes — no global load
//   sits inside the search.
// nbounds up to 2^24 - 1: LDS holds a COARSE table, every 2^s-th bound
//   (coarse[j] = bounds[(j+1)*2^s - 1], at most 4095 entries). Its search
//   yields q with bounds[q*2^s - 1] <= key < bounds[(q+1)*2^s - 1], and at
//   most s length-bounded probes into the global table (L2 / Infinity
//   Cache resident: 128 MB at the 2^24 cap, usually far less) finish it.
//   s == 0 is the first case: one code path serves both.
//
// The LDS table is padded to a power of two with all-ones sentinels. A
// sentinel compares `<= key` for key == 2^64 - 1, so the coarse count is
// clamped to the number of real entries.

#include "common.h"
#include "hipshuffle.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int BND_BLOCK = 256;
constexpr uint32_t BND_MAX_LDS = 4096;        // LDS table entries (32 KB)
constexpr uint32_t BND_MAX_BOUNDS = (1u << 24) - 1;
constexpr uint32_t BND_MAX_GRID = 1024;       // 4 blocks on each of 256 CUs

// Record loads and the pair store have the shape of extract_pairs_kernel
// (kernels.hip): 4-byte-aligned loads, grid-stride loop, one 16-byte store.
__global__ __launch_bounds__(BND_BLOCK) void extract_pairs_bounds_kernel(
    const uint8_t* __restrict__ recs, uint64_t n, uint32_t rec_bytes,
    uint32_t key_bytes, uint64_t* __restrict__ pairs,
    const uint64_t* __restrict__ bounds, uint32_t nbounds,
    uint32_t ncoarse /* nbounds >> s */, uint32_t lds_log2 /* table = 2^.. */,
    uint32_t s /* coarse stride log2 */, uint64_t idx_base) {
  extern __shared__ uint64_t bnd_tab[];
  const uint32_t P = 1u << lds_log2;
  for (uint32_t i = threadIdx.x; i < P; i += BND_BLOCK)
    bnd_tab[i] = i < ncoarse ? bounds[(((uint64_t)i + 1) << s) - 1]
                             : ~0ull;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * BND_BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BND_BLOCK + threadIdx.x; e < n;
       e += stride) {
    const uint8_t* p = recs + e * rec_bytes;
    uint32_t lo = *reinterpret_cast<const uint32_t*>(p);
    uint32_t hi = *reinterpret_cast<const uint32_t*>(p + 4);
    const uint64_t key = ((uint64_t)hi << 32) | lo;
    uint64_t aux = idx_base + e;
    if (key_bytes > 8) {
      uint16_t klo = (uint16_t)(*reinterpret_cast<const uint32_t*>(p + 8));
      aux |= (uint64_t)klo << 48;
    }
    // coarse: count of table entries <= key, at most P - 1
    uint32_t q = 0;
    for (uint32_t step = P >> 1; step; step >>= 1)
      q += bnd_tab[q + step - 1] <= key ? step : 0;
    q = min(q, ncoarse);
    // fine: bounds[base .. base + 2^s - 2], cut off at nbounds
    const uint32_t base = q << s;
    uint32_t f = 0;
    for (uint32_t step = (1u << s) >> 1; step; step >>= 1) {
      const uint32_t i = base + f + step - 1;
      f += (i < nbounds && bounds[i] <= key) ? step : 0;
    }
    reinterpret_cast<ulonglong2*>(pairs)[e] =
        ulonglong2{(uint64_t)(base + f), aux};
  }
}

void extract_pairs_bounds(uintptr_t recs, uint64_t n, uint32_t rec_bytes,
                          uint32_t key_bytes, uintptr_t pairs,
                          uintptr_t bounds, uint32_t nbounds,
                          uintptr_t stream, uint64_t idx_base) {
  if (rec_bytes % 4 || rec_bytes < 8)
    throw std::runtime_error("rec_bytes must be a multiple of 4, >= 8");
  if (key_bytes != 8 && key_bytes != 10)
    throw std::runtime_error("key_bytes must be 8 or 10");
  if (key_bytes > 8 && rec_bytes < 12)
    throw std::runtime_error("10-byte keys need rec_bytes >= 12");
  if (n >> 48) throw std::runtime_error("record count exceeds 2^48");
  if ((idx_base + n) >> 48)
    throw std::runtime_error("idx_base + n exceeds 2^48");
  if (nbounds > BND_MAX_BOUNDS)
    throw std::runtime_error("nbounds exceeds 2^24 - 1");
  if (nbounds && !bounds) throw std::runtime_error("bounds is null");
  uint32_t s = 0;
  while ((nbounds >> s) >= BND_MAX_LDS) ++s;
  const uint32_t ncoarse = nbounds >> s;        // <= 4095
  uint32_t lds_log2 = 0;                        // 2^lds_log2 >= ncoarse + 1
  while ((1u << lds_log2) <= ncoarse) ++lds_log2;
  auto st = reinterpret_cast<hipStream_t>(stream);
  uint32_t grid = (uint32_t)min((n + BND_BLOCK - 1) / BND_BLOCK,
                                (uint64_t)BND_MAX_GRID);
  hipLaunchKernelGGL(extract_pairs_bounds_kernel, dim3(grid ? grid : 1),
                     dim3(BND_BLOCK), sizeof(uint64_t) << lds_log2, st,
                     reinterpret_cast<const uint8_t*>(recs), n, rec_bytes,
                     key_bytes, reinterpret_cast<uint64_t*>(pairs),
                     reinterpret_cast<const uint64_t*>(bounds), nbounds,
                     ncoarse, lds_log2, s, idx_base);
  HIP_CHECK(hipGetLastError());
}

}  // namespace hipshuffle
