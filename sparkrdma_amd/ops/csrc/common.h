// Common helpers for the hipshuffle native library (MI355X / gfx950).
//
// Replaces what libdisni.so + libibverbs did for the reference
// (SURVEY.md §2.3): memory "registration" is hipMalloc + hipIpcGetMemHandle,
// one-sided READ is an xGMI peer copy on a dedicated stream.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      throw std::runtime_error(std::string("HIP error at ") + __FILE__ +    \
                               ":" + std::to_string(__LINE__) + ": " +      \
                               hipGetErrorString(_e) + " in " #expr);       \
    }                                                                       \
  } while (0)

namespace hipshuffle {

constexpr int kWave = 64;  // CDNA wavefront width — NOT 32

// #{ r < n : arr[r] < key } (STRICT) or #{ r < n : arr[r] <= key } over a
// sorted array, by ONE WHOLE WAVE: every step cuts the candidates into 64
// chunks, lane l tests the last element of chunk l, and the ballot's
// popcount names the chunk that holds the boundary — 64-ary narrowing, 4
// dependent loads for 2^24 elements instead of 24. All 64 lanes must call
// it with the same arguments.
template <bool STRICT>
__device__ __forceinline__ uint32_t wave_count_below(
    const uint64_t* __restrict__ arr, uint32_t n, uint64_t key,
    uint32_t lane) {
  uint32_t lo = 0, len = n;               // the count lies in [lo, lo + len]
  while (len) {
    const uint32_t step = (len + kWave - 1) / kWave;
    const uint32_t end = lo + len;
    // (lane + 1) * step <= 64 * ceil(2^31 / 64): no u32 overflow
    const uint32_t idx = lo + (lane + 1) * step - 1;
    bool below = false;
    if (idx < end) below = STRICT ? arr[idx] < key : arr[idx] <= key;
    const uint32_t c = (uint32_t)__popcll(__ballot(below));
    // chunks 0..c-1 are below; chunk c's last element, if it exists, is not
    lo += c * step;
    len = min(step - 1, end - lo);
  }
  return lo;
}

constexpr uint64_t AUX_IDX_MASK = (1ull << 48) - 1;  // aux = keylo16<<48 | idx

// Where record idx of a pair's aux word lives. Record indices are positions
// in the reader's (virtual) arena; the records themselves may sit in
// several places — a reader that takes its local blocks in place leaves
// them in the shuffle's HBM blocks and copies only the rest into the arena
// (reader.py record_segments). The caller passes a device table of nsegs
// entries sorted by first_rec that cover [0, n) without gap or overlap;
// record idx is record (idx - first_rec) of the LAST entry with
// first_rec <= idx, counted from that entry's base. nsegs == 0: the
// records are contiguous from `recs`, the plain address arithmetic, behind
// a branch that is uniform for the whole grid (nsegs is a kernel argument).
//
// The table is searched in global memory: the flagship job has 86 entries,
// one per fetch (16 bytes each, read by every block, so it stays in L2 and
// the vector L1; 7 search steps cost its final pass 0.8 %,
// profiles/r08_inplace_local_records.md), and the search runs once per
// slot in the staging
// loops, ahead of the record loads it addresses — copy_record_words never
// sees it. An LDS copy would cap the table (the fused pass has under 4 KB
// to spare before it loses its second resident block).
struct RecSegment {
  uint64_t first_rec;    // index of the segment's first record
  const uint32_t* base;  // first word of that record
};

__device__ __forceinline__ const uint32_t* record_src(
    const uint32_t* __restrict__ recs, const RecSegment* __restrict__ segs,
    uint32_t nsegs, uint64_t idx, uint32_t w4) {
  if (nsegs == 0) return recs + idx * w4;
  // segs[lo].first_rec <= idx < segs[hi].first_rec (segs[0].first_rec is
  // 0, hi == nsegs stands for +inf): only entries in [1, nsegs) are read
  uint32_t lo = 0, hi = nsegs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (segs[mid].first_rec <= idx)
      lo = mid;
    else
      hi = mid;
  }
  const RecSegment s = segs[lo];
  return s.base + (idx - s.first_rec) * w4;
}

inline int device_count() {
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  return n;
}

}  // namespace hipshuffle
