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

inline int device_count() {
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  return n;
}

}  // namespace hipshuffle
