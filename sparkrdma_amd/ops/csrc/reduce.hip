// Segmented reduce over key-sorted 16-byte (u64 key, u64 value) AoS pairs
// for MI355X (gfx950) — the keyed-aggregation primitive of both shuffle
// sides: map-side combine in the writer, merge/aggregate in the reader
// (the reference's combineValuesByKey / combineCombinersByKey branches,
// RdmaShuffleReader.scala:83-96).
//
// Element i is a HEAD iff i == 0 or key[i] != key[i-1] (all 64 bits). A run
// is a head and the non-heads after it. Output is SoA, one (key, reduction)
// per run in input order. The kernel looks at adjacency only.
//
// Scheme — two launches of ONE kernel template, a scan of per-tile head
// counts between them (plumbing in ops/radix.py):
//
//   tile = 256 threads x 8 records, loaded lane-linear (coalesced dwordx4),
//   transposed through padded LDS so that each thread owns 8 consecutive
//   records.
//
//   count pass   heads[b] = heads in tile b
//                lead[b]  = reduction of the records before tile b's first
//                           head (the whole tile when it has none, the
//                           identity when record 0 is a head)
//   scan         base[b]  = exclusive sum of heads
//   emit pass    the same in-tile segmented reduction (thread-serial over
//                its records, wave64 segmented scan with __shfl_up, four
//                wave aggregates through LDS). Every head writes its key
//                at base[b] + rank; whoever closes a run that began in
//                this tile writes its value. The tile's LAST run is open
//                at the tile's end: wave 0 walks forward over lead[b+1],
//                lead[b+2], ... 64 tiles per step, folds them in and
//                stops after the first tile that holds a head.
//
// No block waits on another block: the walk reads what the count LAUNCH
// wrote, never what a concurrent block writes. Every combine order is fixed
// by (n, tile geometry) alone, so sum_f64 is bit-reproducible; there are no
// atomics. Total walk work is O(tiles): a lead is folded by exactly one
// walker, plus at most 63 discarded loads per step.
//
// Identities: 0 for sum/count, INT64_MAX / INT64_MIN for min / max, and
// -0.0 for sum_f64 (-0.0 + x == x for every x including both zeros, so
// folding an empty lead never changes a bit of the result).

#include "common.h"
#include "hipshuffle.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int RBK_BLOCK = 256;
constexpr int RBK_ITEMS = 8;
constexpr int RBK_TILE = RBK_BLOCK * RBK_ITEMS;
constexpr int RBK_WAVES = RBK_BLOCK / kWave;

enum { RBK_SUM = 0, RBK_SUM_F64 = 1, RBK_COUNT = 2, RBK_MIN = 3, RBK_MAX = 4 };

template <int OP>
__device__ __forceinline__ uint64_t rbk_identity() {
  if constexpr (OP == RBK_SUM_F64) return 0x8000000000000000ull;  // -0.0
  else if constexpr (OP == RBK_MIN) return 0x7fffffffffffffffull;
  else if constexpr (OP == RBK_MAX) return 0x8000000000000000ull;
  else return 0;
}

template <int OP>
__device__ __forceinline__ uint64_t rbk_op(uint64_t a, uint64_t b) {
  if constexpr (OP == RBK_SUM_F64) {
    return (uint64_t)__double_as_longlong(
        __longlong_as_double((long long)a) + __longlong_as_double((long long)b));
  } else if constexpr (OP == RBK_MIN) {
    return (int64_t)a < (int64_t)b ? a : b;
  } else if constexpr (OP == RBK_MAX) {
    return (int64_t)a > (int64_t)b ? a : b;
  } else {
    return a + b;
  }
}

__device__ __forceinline__ uint64_t rbk_shfl_up(uint64_t v, int d) {
  return (uint64_t)__shfl_up((unsigned long long)v, d, kWave);
}

// EMIT == false: the count pass (writes heads[b], lead[b]).
// EMIT == true : the emit pass (reads heads, lead, base; writes out_*).
template <int OP, bool EMIT>
__global__ __launch_bounds__(RBK_BLOCK) void reduce_by_key_kernel(
    const ulonglong2* __restrict__ pairs, uint32_t n, uint32_t* heads,
    uint64_t* lead, const uint64_t* __restrict__ base,
    uint64_t* __restrict__ out_keys, uint64_t* __restrict__ out_vals) {
  // record r sits in slot r + r/8: a thread's 8 records start at slot 9t,
  // a 144-byte stride that keeps the ds_read_b128 lane groups off each
  // other's banks
  __shared__ ulonglong2 stage[RBK_TILE + RBK_TILE / 8];
  __shared__ uint64_t w_val[RBK_WAVES];
  __shared__ uint32_t w_flag[RBK_WAVES];
  __shared__ uint32_t w_heads[RBK_WAVES];

  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const uint32_t b = blockIdx.x, nb = gridDim.x;
  const uint64_t tile0 = (uint64_t)b * RBK_TILE;
  const uint64_t ident = rbk_identity<OP>();

#pragma unroll
  for (int j = 0; j < RBK_ITEMS; ++j) {
    const uint32_t r = j * RBK_BLOCK + t;
    if (tile0 + r < n) stage[r + (r >> 3)] = pairs[tile0 + r];
  }
  __syncthreads();

  const uint64_t i0 = tile0 + (uint64_t)t * RBK_ITEMS;
  const int m = i0 >= n ? 0
                        : (n - i0 < RBK_ITEMS ? (int)(n - i0) : RBK_ITEMS);
  uint64_t k[RBK_ITEMS], v[RBK_ITEMS];
#pragma unroll
  for (int j = 0; j < RBK_ITEMS; ++j) {
    if (j < m) {
      const ulonglong2 rec = stage[9 * t + j];
      k[j] = rec.x;
      v[j] = OP == RBK_COUNT ? 1 : rec.y;
    } else {
      k[j] = 0;
      v[j] = ident;
    }
  }
  uint64_t prev = 0;
  if (m > 0 && i0 > 0) prev = t ? stage[9 * t - 2].x : pairs[tile0 - 1].x;

  // head flags and this thread's head count
  uint32_t hmask = 0;
#pragma unroll
  for (int j = 0; j < RBK_ITEMS; ++j) {
    if (j < m) {
      const bool h = j ? k[j] != k[j - 1] : (i0 == 0 || k[0] != prev);
      hmask |= (uint32_t)h << j;
    }
  }
  const uint32_t hc = __popc(hmask);

  // exclusive head count before this thread, and the tile's total
  uint32_t inc = hc;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t u = __shfl_up(inc, d, kWave);
    if (lane >= (uint32_t)d) inc += u;
  }
  if (lane == kWave - 1) w_heads[wv] = inc;
  __syncthreads();
  uint32_t excl = inc - hc, H = 0;
#pragma unroll
  for (int w = 0; w < RBK_WAVES; ++w) {
    if ((uint32_t)w < wv) excl += w_heads[w];
    H += w_heads[w];
  }
  const uint64_t rank0 = EMIT ? base[b] + excl : 0;

  // thread-serial: prefix = records before the first head, acc ends as the
  // open suffix (or the thread's total when it holds no head); runs that
  // open and close inside the thread are written here
  uint64_t acc = ident, prefix = ident;
  uint32_t seen = 0;
#pragma unroll
  for (int j = 0; j < RBK_ITEMS; ++j) {
    if (j < m) {
      if ((hmask >> j) & 1) {
        if (seen == 0) {
          prefix = acc;
        } else if (EMIT) {
          out_vals[rank0 + seen - 1] = acc;
        }
        if (EMIT) out_keys[rank0 + seen] = k[j];
        acc = v[j];
        ++seen;
      } else {
        acc = rbk_op<OP>(acc, v[j]);
      }
    }
  }

  // wave64 segmented inclusive scan: a thread with a head starts a segment
  uint64_t sv = acc;
  uint32_t sf = hc > 0;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t uv = rbk_shfl_up(sv, d);
    const uint32_t uf = __shfl_up(sf, d, kWave);
    if (lane >= (uint32_t)d) {
      if (!sf) sv = rbk_op<OP>(uv, sv);
      sf |= uf;
    }
  }
  uint64_t xv = rbk_shfl_up(sv, 1);
  uint32_t xf = __shfl_up(sf, 1, kWave);
  if (lane == 0) {
    xv = ident;
    xf = 0;
  }
  if (lane == kWave - 1) {
    w_val[wv] = sv;
    w_flag[wv] = sf;
  }
  __syncthreads();
  // waves before this one, left to right; `tail` folds all of them: the
  // reduction of the tile's open last run (of the whole tile when H == 0)
  uint64_t cv = ident, tail = ident;
#pragma unroll
  for (int w = 0; w < RBK_WAVES; ++w) {
    const uint64_t wvv = w_val[w];
    tail = w_flag[w] ? wvv : rbk_op<OP>(tail, wvv);
    if ((uint32_t)w + 1 == wv) cv = tail;
  }
  const uint64_t carry = xf ? xv : rbk_op<OP>(cv, xv);

  if (hc > 0) {
    // closes the run that was open at this thread's first head
    const uint64_t closed = rbk_op<OP>(carry, prefix);
    if (excl > 0) {
      if (EMIT) out_vals[rank0 - 1] = closed;
    } else if (!EMIT) {
      lead[b] = closed;       // began before this tile: someone else's run
    }
  }
  if (!EMIT) {
    if (t == 0) {
      heads[b] = H;
      if (H == 0) lead[b] = tail;
    }
    return;
  }

  // forward walk by wave 0: the tile's last run, open at the tile's end
  if (wv != 0 || H == 0) return;
  uint64_t run = tail;
  for (uint64_t s0 = (uint64_t)b + 1; s0 < nb; s0 += kWave) {
    const uint64_t tb = s0 + lane;
    const bool in = tb < nb;
    const uint32_t h = in ? heads[tb] : 0;
    uint64_t l = in ? lead[tb] : ident;
    const unsigned long long bal = __ballot(in && h > 0);
    const uint32_t first = bal ? (uint32_t)__ffsll((long long)bal) - 1 : kWave;
    if (lane > first) l = ident;
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
      const uint64_t o =
          (uint64_t)__shfl_down((unsigned long long)l, d, kWave);
      l = rbk_op<OP>(l, o);
    }
    run = rbk_op<OP>(run, (uint64_t)__shfl((unsigned long long)l, 0, kWave));
    if (bal) break;
  }
  if (lane == 0) out_vals[base[b] + H - 1] = run;
}

// ---------------------------------------------------------------------------
// host wrappers
//
// workspace layout for nb = ceil(n / tile) tiles, 8-byte aligned:
//   [lead u64 x nb][base u64 x nb][heads u32 x nb]
// The caller fills base[] (exclusive scan of heads) between the two calls.

static inline uint32_t rbk_tiles(uint32_t n) {
  return (uint32_t)(((uint64_t)n + RBK_TILE - 1) / RBK_TILE);
}

int reduce_by_key_tile() { return RBK_TILE; }

size_t reduce_by_key_workspace_bytes(uint32_t n) {
  const size_t nb = rbk_tiles(n);
  return nb * 16 + ((nb * 4 + 7) & ~(size_t)7);
}

template <bool EMIT>
static void rbk_launch(uintptr_t pairs, uint32_t n, int op, uintptr_t ws,
                       uintptr_t out_keys, uintptr_t out_vals,
                       uintptr_t stream) {
  if (n == 0) return;
  if (op < 0 || op > RBK_MAX)
    throw std::invalid_argument("reduce_by_key: unknown op code");
  if ((pairs & 15) || (ws & 7) || (out_keys & 7) || (out_vals & 7))
    throw std::invalid_argument("reduce_by_key: misaligned buffer");
  auto s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t nb = rbk_tiles(n);
  auto* p = reinterpret_cast<const ulonglong2*>(pairs);
  auto* lead = reinterpret_cast<uint64_t*>(ws);
  auto* base = lead + nb;
  auto* heads = reinterpret_cast<uint32_t*>(base + nb);
  auto* ok = reinterpret_cast<uint64_t*>(out_keys);
  auto* ov = reinterpret_cast<uint64_t*>(out_vals);
#define RBK_CASE(OP)                                                        \
  case OP:                                                                  \
    hipLaunchKernelGGL((reduce_by_key_kernel<OP, EMIT>), dim3(nb),          \
                       dim3(RBK_BLOCK), 0, s, p, n, heads, lead, base, ok,  \
                       ov);                                                 \
    break;
  switch (op) {
    RBK_CASE(RBK_SUM)
    RBK_CASE(RBK_SUM_F64)
    RBK_CASE(RBK_COUNT)
    RBK_CASE(RBK_MIN)
    RBK_CASE(RBK_MAX)
  }
#undef RBK_CASE
  HIP_CHECK(hipGetLastError());
}

void reduce_by_key_count(uintptr_t pairs, uint32_t n, int op, uintptr_t ws,
                         uintptr_t stream) {
  rbk_launch<false>(pairs, n, op, ws, 0, 0, stream);
}

void reduce_by_key_emit(uintptr_t pairs, uint32_t n, int op, uintptr_t ws,
                        uintptr_t out_keys, uintptr_t out_vals,
                        uintptr_t stream) {
  rbk_launch<true>(pairs, n, op, ws, out_keys, out_vals, stream);
}

}  // namespace hipshuffle
