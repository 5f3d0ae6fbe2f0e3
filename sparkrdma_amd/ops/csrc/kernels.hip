// CDNA4 (gfx950) shuffle kernels: radix bucket-scatter machinery.
//
// One primitive serves both hot paths (SURVEY.md §2.3 "new GPU kernels"):
//   * map-side partition+serialize: digit = top log2(R) key bits; the
//     scatter writes keys/values STRAIGHT into their final positions in
//     HBM block buffers (per-digit destination base pointers) — no
//     intermediate file, replacing Spark's CPU sort-shuffle writer
//     (reference RdmaWrapperShuffleWriter.scala:83-102).
//   * reduce-side LSD radix sort: 8-bit digits, ping-pong buffers.
//
// Design (MI355X-first, not a CUDA port):
//   * wave = 64: rank computation is a 64-lane ballot multi-split
//     (8..12 __ballot()s of 64 bits), per-wave LDS counters — no atomics.
//   * stability: wave w owns the contiguous element chunk
//     [tile + w*64*ITEMS, ...), iterated lane-major, so block order ==
//     memory order and ranks are stable.
//   * scattered global writes are coalesced through an LDS exchange
//     (elements digit-sorted in LDS, then written out linearly — each
//     digit's run is a contiguous global write burst).
//   * partition path: 3-kernel (hist -> hierarchical scan -> scatter;
//     row-major [nb][ND] hist so every access is thread==digit coalesced)
//     because the host must see counts to lay out HBM blocks first
//     (wide records into at most 256 partitions: counts, then ONE fused
//     onesweep pass — see 'wide-record machinery').
//   * sort path: onesweep — one kernel per pass with decoupled lookback
//     (u64 flag|count agent-scope descriptors), AoS records, deferred
//     walk; selectable hist+scan mode kept for A/B.
//
// Limits: n < 2^32 elements per call; ONE pass covers 2^4..2^12 LDS
// digits — arbitrary partition counts come from the partition funcs
// (PartFunc 2/3) and, above 4096, the writer's two-level pid radix.

#include "common.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int BLOCK = 256;        // 4 waves
constexpr int ITEMS = 16;         // elements per thread
constexpr int TILE = BLOCK * ITEMS;  // 4096 elements per workgroup
constexpr int NW = BLOCK / kWave;    // waves per block

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    uint32_t t = __shfl_up(v, d);
    if ((threadIdx.x & (kWave - 1)) >= (unsigned)d) v += t;
  }
  return v;
}

// Exclusive scan of arr[nd] in LDS (nd pow2); sums: >=BS u32.
template <int BS = BLOCK>
__device__ void block_exscan(uint32_t* arr, uint32_t* sums, int nd) {
  const int tid = threadIdx.x;
  const int per = (nd + BS - 1) / BS;  // >= 1
  const int lo = tid * per;
  uint32_t run = 0;
#pragma unroll 1
  for (int k = 0; k < per; ++k) {
    int idx = lo + k;
    uint32_t v = idx < nd ? arr[idx] : 0;
    if (idx < nd) arr[idx] = run;
    run += v;
  }
  sums[tid] = run;
  __syncthreads();
  if (tid < kWave) {
    uint32_t off = 0;
#pragma unroll 1
    for (int c = 0; c < BS / kWave; ++c) {
      uint32_t v = sums[c * kWave + tid];
      uint32_t inc = wave_inclusive_scan(v);
      sums[c * kWave + tid] = off + inc - v;
      off += __shfl(inc, kWave - 1);
    }
  }
  __syncthreads();
  uint32_t base = sums[tid];
#pragma unroll 1
  for (int k = 0; k < per; ++k) {
    int idx = lo + k;
    if (idx < nd) arr[idx] += base;
  }
  __syncthreads();
}

// splitmix64 finalizer step — bit-identical to partitioner.HashPartitioner
// so GPU hash partitioning matches the CPU oracle exactly.
__device__ __forceinline__ uint64_t hash_mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  return k;
}

// Partition functions (the `func` runtime param of hist/scatter). 0/1 are
// the r01 bit-extraction modes; 2/3 lift the pow2-only restriction
// (VERDICT r01 missing item 7): any R <= 2^12 via multiply-high range
// partitioning (pid = floor(key * R / 2^64), exactly the CPU
// RangePartitioner with ceil bounds) or hash-mod. The digit still fits
// the pow2 LDS counter layout (ND = next pow2 >= R).
enum PartFunc : int {
  kPartBits = 0,      // (key >> shift) & mask
  kPartHashBits = 1,  // (mix(key) >> shift) & mask   (== mod for pow2 R)
  kPartRange = 2,     // mulhi(key, R)                 (any R)
  kPartHashMod = 3,   // mix(key) % R                  (any R)
};

__device__ __forceinline__ uint32_t digit_of(uint64_t k, int shift,
                                             uint32_t mask, int func,
                                             uint32_t nparts) {
  switch (func) {
    default:
    case kPartBits: return (uint32_t)(k >> shift) & mask;
    case kPartHashBits: return (uint32_t)(hash_mix64(k) >> shift) & mask;
    case kPartRange:
      return (uint32_t)(((unsigned __int128)k * nparts) >> 64);
    case kPartHashMod: return (uint32_t)(hash_mix64(k) % nparts);
  }
}

// Match from PRE-COMPUTED per-bit ballots (register votes) — lets rank
// logic reuse one iteration's ballots against another iteration's digits.
template <int PBITS>
__device__ __forceinline__ uint64_t match_votes(const uint64_t* v,
                                                uint64_t vm, uint32_t d) {
  uint64_t m = vm;
#pragma unroll
  for (int b = 0; b < PBITS; ++b) m &= ((d >> b) & 1) ? v[b] : ~v[b];
  return m;
}

// 64-lane multi-split: lanes with equal `digit` (among `validmask` lanes).
template <int NBITS>
__device__ __forceinline__ uint64_t match_lanes(uint32_t digit,
                                                uint64_t validmask) {
  uint64_t match = validmask;
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    uint64_t vote = __ballot((digit >> b) & 1);
    match &= ((digit >> b) & 1) ? vote : ~vote;
  }
  return match;
}

// ---------------------------------------------------------------------------
// Kernel 1: per-block digit histogram. hist layout: [nb][ND] (row-major) —
// hist writes, scan passes and the scatter's prefix preload are all
// coalesced across the 256 threads (thread==digit lane).

template <int NBITS>
__global__ __launch_bounds__(BLOCK) void radix_hist_kernel(
    const uint64_t* __restrict__ keys, uint32_t n, int shift,
    uint32_t* __restrict__ hist, uint32_t nb, int func,
    int in_stride = 1, uint32_t nparts = 0) {
  constexpr int ND = 1 << NBITS;
  extern __shared__ char smem_raw[];
  uint32_t* counters = reinterpret_cast<uint32_t*>(smem_raw);  // [NW][ND]
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  const uint64_t tile_start = (uint64_t)b * TILE;
  uint32_t* my = counters + wave * ND;
  for (int d = tid; d < NW * ND; d += BLOCK) counters[d] = 0;
  __syncthreads();

  const uint64_t chunk = tile_start + (uint64_t)wave * (ITEMS * kWave);
  // loads issued in their own unrolled loop so they are all in flight
  // before the serial LDS counter chain (same fix as the sort pass:
  // phase A 11.4 -> 8.2 us/block)
  uint64_t key_reg[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    key_reg[i] = e < n ? keys[e * in_stride] : 0;
  }
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    bool valid = e < n;
    uint32_t d = digit_of(key_reg[i], shift, ND - 1, func, nparts);
    uint64_t vm = __ballot(valid);
    if (valid) {
      uint64_t match = match_lanes<NBITS>(d, vm);
      uint64_t lt = (1ull << lane) - 1;
      if ((match & lt) == 0) my[d] += (uint32_t)__popcll(match);
    }
  }
  __syncthreads();
  for (int d = tid; d < ND; d += BLOCK) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += counters[w * ND + d];
    hist[(uint64_t)b * ND + d] = s;
  }
}

// ---------------------------------------------------------------------------
// Kernel 2: hierarchical scan of hist[nb][ND] along the block axis per
// digit. Three coalesced passes (thread == digit lane, rows iterated
// serially): K2a per-chunk digit sums -> K2b single-block scan over
// chunks (+ digit totals) -> K2c rewrite rows as running prefixes.
// Cross-chunk sums travel through global memory between kernels — kernel
// boundaries are the release/acquire, no in-launch cross-XCD protocol
// needed. The matrix is ~2% of a pass's traffic; the naive per-column
// chained scan was O(nb) *latency* (4.5 ms at nb=655k).

template <int ND>
__global__ __launch_bounds__(BLOCK) void scan_chunk_sums_kernel(
    const uint32_t* __restrict__ hist, uint32_t nb, uint32_t chunk_rows,
    uint32_t* __restrict__ partial) {
  const uint32_t c = blockIdx.x;
  const uint32_t lo = c * chunk_rows, hi = min(lo + chunk_rows, nb);
  for (int d = threadIdx.x; d < ND; d += BLOCK) {
    uint32_t run = 0;
    for (uint32_t r = lo; r < hi; ++r) run += hist[(uint64_t)r * ND + d];
    partial[(uint64_t)c * ND + d] = run;
  }
}

template <int ND>
__global__ __launch_bounds__(BLOCK) void scan_chunks_kernel(
    uint32_t* __restrict__ partial, uint32_t chunks,
    uint32_t* __restrict__ totals) {
  for (int d = threadIdx.x; d < ND; d += BLOCK) {
    uint32_t run = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
      uint32_t v = partial[(uint64_t)c * ND + d];
      partial[(uint64_t)c * ND + d] = run;
      run += v;
    }
    totals[d] = run;
  }
}

template <int ND>
__global__ __launch_bounds__(BLOCK) void scan_rewrite_kernel(
    uint32_t* __restrict__ hist, uint32_t nb, uint32_t chunk_rows,
    const uint32_t* __restrict__ partial) {
  const uint32_t c = blockIdx.x;
  const uint32_t lo = c * chunk_rows, hi = min(lo + chunk_rows, nb);
  for (int d = threadIdx.x; d < ND; d += BLOCK) {
    uint32_t run = partial[(uint64_t)c * ND + d];
    for (uint32_t r = lo; r < hi; ++r) {
      uint32_t v = hist[(uint64_t)r * ND + d];
      hist[(uint64_t)r * ND + d] = run;
      run += v;
    }
  }
}

static inline uint32_t scan_chunk_rows(uint32_t nb) {
  // target ~2048 blocks; at least 64 rows per chunk to amortize
  uint32_t c = (nb + 2047) / 2048;
  return c < 64 ? 64 : c;
}

// ---------------------------------------------------------------------------
// Kernel 2b (sort path): turn totals into per-digit destination pointers
// inside the ping-pong output buffers — keeps the whole sort device-side
// (no host round trip between passes).

template <int NBITS>
__global__ void radix_digit_bases_kernel(const uint32_t* __restrict__ totals,
                                         uint64_t out_keys, uint64_t out_vals,
                                         uint64_t* __restrict__ key_dst,
                                         uint64_t* __restrict__ val_dst) {
  constexpr int ND = 1 << NBITS;
  __shared__ uint32_t arr[ND];
  __shared__ uint32_t sums[BLOCK];
  const int tid = threadIdx.x;
  for (int d = tid; d < ND; d += BLOCK) arr[d] = totals[d];
  __syncthreads();
  block_exscan(arr, sums, ND);
  for (int d = tid; d < ND; d += BLOCK) {
    key_dst[d] = out_keys + (uint64_t)arr[d] * 8;
    val_dst[d] = out_vals ? out_vals + (uint64_t)arr[d] * 8 : 0;
  }
}

// ---------------------------------------------------------------------------
// Kernel 3: rank + LDS exchange + scatter to per-digit destinations.

template <int NBITS, bool HAS_VAL>
__global__ __launch_bounds__(BLOCK) void radix_scatter_kernel(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
    uint32_t n, int shift, const uint32_t* __restrict__ hist, uint32_t nb,
    const uint64_t* __restrict__ key_dst, const uint64_t* __restrict__ val_dst,
    int func, int aos_out, int in_stride = 1, uint32_t nparts = 0) {
  constexpr int ND = 1 << NBITS;
  extern __shared__ char smem_raw[];
  // layout: exchange u64[TILE] | counters u32[NW][ND] | start u32[ND]
  //         | pref u32[ND] | sums u32[BLOCK]
  uint64_t* exch = reinterpret_cast<uint64_t*>(smem_raw);
  uint32_t* counters = reinterpret_cast<uint32_t*>(exch + TILE);
  uint32_t* start = counters + NW * ND;
  uint32_t* pref = start + ND;
  uint32_t* sums = pref + ND;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  const uint64_t tile_start = (uint64_t)b * TILE;
  const uint32_t tile_n =
      (uint32_t)min((uint64_t)TILE, (uint64_t)n - tile_start);
  uint32_t* my = counters + wave * ND;

  for (int d = tid; d < NW * ND; d += BLOCK) counters[d] = 0;
  // preload this block's cross-block digit prefixes (coalesced row read)
  for (int d = tid; d < ND; d += BLOCK) pref[d] = hist[(uint64_t)b * ND + d];
  __syncthreads();

  // phase A: per-element (digit, rank within wave&digit), stable;
  // loads split from the serial LDS counter chain (see sort pass)
  uint64_t key_reg[ITEMS];
  uint32_t rank_reg[ITEMS];
  uint32_t dig_reg[ITEMS];
  const uint64_t chunk = tile_start + (uint64_t)wave * (ITEMS * kWave);
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    key_reg[i] = e < n ? keys[e * in_stride] : 0;
  }
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    bool valid = e < n;
    uint32_t d = digit_of(key_reg[i], shift, ND - 1, func, nparts);
    dig_reg[i] = d;
    uint64_t vm = __ballot(valid);
    uint32_t r = 0;
    if (valid) {
      uint64_t match = match_lanes<NBITS>(d, vm);
      uint64_t lt = (1ull << lane) - 1;
      uint32_t rank_in_iter = (uint32_t)__popcll(match & lt);
      uint32_t c = my[d];
      r = c + rank_in_iter;
      if (rank_in_iter == 0) my[d] = c + (uint32_t)__popcll(match);
    }
    rank_reg[i] = r;
  }
  __syncthreads();

  // scan waves per digit; block totals into start[]
  for (int d = tid; d < ND; d += BLOCK) {
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      uint32_t t = counters[w * ND + d];
      counters[w * ND + d] = run;
      run += t;
    }
    start[d] = run;
  }
  __syncthreads();
  block_exscan(start, sums, ND);  // start[d] = block-local digit start

  // LDS exchange: keys to digit-sorted local order
#pragma unroll 1
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    if (e < n) {
      uint32_t d = dig_reg[i];
      uint32_t j = start[d] + my[d] + rank_reg[i];
      rank_reg[i] = j;  // reuse: now holds local sorted position
      exch[j] = key_reg[i];
    }
  }
  __syncthreads();

  // linear write-out of keys; remember (digit, global offset) per slot
  uint32_t out_d[ITEMS];
  uint32_t out_off[ITEMS];
#pragma unroll 1
  for (int i = 0; i < ITEMS; ++i) {
    uint32_t j = i * BLOCK + tid;
    if (j < tile_n) {
      uint64_t k = exch[j];
      uint32_t d = digit_of(k, shift, ND - 1, func, nparts);
      uint32_t off = (pref[d] + (j - start[d])) << aos_out;
      out_d[i] = d;
      out_off[i] = off;
      reinterpret_cast<uint64_t*>(key_dst[d])[off] = k;
    }
  }
  if (HAS_VAL) {
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < ITEMS; ++i) {
      uint64_t e = chunk + (uint64_t)i * kWave + lane;
      if (e < n) exch[rank_reg[i]] = vals[e * in_stride];
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < ITEMS; ++i) {
      uint32_t j = i * BLOCK + tid;
      if (j < tile_n)
        reinterpret_cast<uint64_t*>(val_dst[out_d[i]])[out_off[i]] = exch[j];
    }
  }
}

// ---------------------------------------------------------------------------
// Batched record copy, shared by gather_records_kernel and the fused final
// sort pass (see 'wide-record machinery' below). The caller stages one
// (source, destination) address pair per record in LDS; the block then
// moves the records one word per lane.

struct GatherSlot {
  const uint32_t* src;  // first word of the record
  uint32_t* dst;        // first word of its destination slot
};

// independent record loads a lane issues before its first store
constexpr int GATHER_BATCH = 8;  // 16: no faster, 90 / 160 VGPRs

// Copy nslots records of w4 words each. Word q of the block is word
// q % w4 of slot q / w4, so a wave-instruction reads 256 consecutive bytes
// of consecutive slots' records and its store is 256 contiguous bytes
// within a destination run. (slot, word) advance by the block-uniform
// step (BS / w4, BS % w4): one division per lane, none per word. Each
// lane issues U loads before its first store, and the loop body is
// branch-free so no wait separates the loads.
//
// Lane mapping: one dword per lane measured FASTER than 16 bytes per lane
// with a narrower tail (100 B = 6 x 16 + 4) — 2.55 vs 4.5 ms for 4 GB of
// 100-byte records, equal at 256 bytes where there is no tail; the tail
// chunks are 4-byte accesses 100 bytes apart
// (profiles/r03_record_movement.md).
//
// INVARIANT (no access outside the record): a lane touches word o of
// slot r only with r < nslots and o < w4, on both sides, and every access
// is exactly one word wide. So it lies inside [record, record + W) on the
// source and inside the record's destination slot on the destination.
template <int BS, int U>
__device__ __forceinline__ void copy_record_words(const GatherSlot* slots,
                                                  uint32_t nslots,
                                                  uint32_t w4) {
  // the addresses come out of LDS: name the global address space, else
  // the accesses lower to flat_load / flat_store
  typedef const __attribute__((address_space(1))) uint32_t* gsrc_t;
  typedef __attribute__((address_space(1))) uint32_t* gdst_t;
  const uint32_t total = nslots * w4;
  const uint32_t dr = BS / w4, dc = BS % w4;
  uint32_t r = threadIdx.x / w4, o = threadIdx.x % w4;
#pragma unroll 1
  for (uint32_t q0 = 0; q0 < total; q0 += BS * U) {
    uint32_t v[U];
    gdst_t dst[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // lanes past the end re-read the block's last word (inside a
      // record) and skip the store below
      const bool ok = q0 + (uint32_t)u * BS + threadIdx.x < total;
      const GatherSlot s = slots[ok ? r : nslots - 1];
      const uint32_t w = ok ? o : w4 - 1;
      v[u] = ((gsrc_t)s.src)[w];
      dst[u] = (gdst_t)s.dst + w;
      o += dc;
      r += dr;
      if (o >= w4) {
        o -= w4;
        ++r;
      }
    }
    // plain cached accesses: streaming (nontemporal) hints measured
    // 252 vs 256 GB/s on the flagship — the L2 reuse between the
    // producing kernels and the copy outweighs the pollution
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (q0 + (uint32_t)u * BS + threadIdx.x < total) *dst[u] = v[u];
  }
}

// ---------------------------------------------------------------------------
// Onesweep path (8-bit digits): one kernel per pass with decoupled
// lookback — removes the per-pass hist read and the scan kernels.
//
// Status word per (block, digit): 2-bit flag | 62-bit count/prefix packed
// in ONE u64, so a single relaxed agent-scope atomic is a complete
// publish (no multi-location ordering; the guide's G16 concerns collapse
// to single-word atomicity; an 8-byte relaxed agent store lowers to an
// sc1 write-through). Agent-scope atomics are cache-coherent across
// XCDs. Blocks take an atomic ticket at start, so a block's predecessors
// in lookback order are already launched -> no deadlock, and the ticket
// determines the tile, so results are placement- and timing-independent.

constexpr uint64_t FLAG_AGG = 1ull << 62;
constexpr uint64_t FLAG_INC = 2ull << 62;
constexpr uint64_t FLAG_MASK = 3ull << 62;
constexpr uint64_t VAL_MASK = (1ull << 62) - 1;

// Serial decoupled-lookback walk for digit `tid`: sum predecessors'
// aggregates back to the nearest inclusive prefix, publish our own
// inclusive, record the exclusive prefix in pref[tid]. (A windowed
// 8-wide variant measured NO faster — the cost is waiting on the
// publish frontier, not load throughput — so the caller overlaps this
// wait with the LDS exchange instead.)
template <int ND>
__device__ __forceinline__ void lookback_walk(
    uint64_t* __restrict__ desc, uint32_t b, int tid, uint64_t my_total,
    uint32_t* __restrict__ pref) {
  uint64_t run = 0;
  for (int64_t j = (int64_t)b - 1; j >= 0;) {
    uint64_t v = __hip_atomic_load(&desc[(uint64_t)j * ND + tid],
                                   __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    if ((v & FLAG_MASK) == 0) {
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    run += v & VAL_MASK;
    if ((v & FLAG_MASK) == FLAG_INC) break;
    --j;
  }
  __hip_atomic_store(&desc[(uint64_t)b * ND + tid],
                     FLAG_INC | (run + my_total), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
  pref[tid] = (uint32_t)run;
}

// Global digit totals of EVERY pass in one read (digit counts are
// order-independent, so pass k's totals can be computed from pass 0's
// input).
template <int MAX_PASSES, int PBITS>
__global__ __launch_bounds__(BLOCK) void onesweep_hist_all_kernel(
    const uint64_t* __restrict__ keys, uint32_t n, int start_bit, int passes,
    uint32_t* __restrict__ totals /* [passes][1<<PBITS] */, int in_stride,
    int word_off = 0) {
  constexpr int PD = 1 << PBITS;
  __shared__ uint32_t cnt[NW][MAX_PASSES * PD];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  for (int i = tid; i < NW * MAX_PASSES * PD; i += BLOCK)
    cnt[0][i] = 0;  // flat zero (cnt rows contiguous)
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + tid; e < n; e += stride) {
    uint64_t k = keys[e * in_stride + word_off];
    for (int p = 0; p < passes; ++p) {
      int sb = start_bit + p * PBITS;
      if (sb > 64 - PBITS) sb = 64 - PBITS;  // last pass re-covers top bits
      uint32_t d = (uint32_t)(k >> sb) & (PD - 1);
      atomicAdd(&cnt[wave][p * PD + d], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < passes * PD; i += BLOCK) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += cnt[w][i];
    if (s) atomicAdd(&totals[i], s);
  }
}

// One LSD pass over an 8-bit digit: each block ranks a tile of BS * IT
// elements, publishes its digit counts, reorders the tile by digit in
// LDS, and writes every digit run to its place in the output, found
// from the per-digit bases in key_dst / val_dst and the lookback prefix.
// AOS = false: keys and vals are separate u64 arrays; the keys go
// through the LDS exchange first, the vals (HAS_VAL) after them.
// AOS = true: elements are interleaved (key, val) 16-byte records — one
// dwordx4 load per element, a pair LDS exchange, ONE 16-byte store per
// element, and 2x-longer digit write bursts (measured: scattered-write
// bandwidth doubles from 128 B to 256 B bursts — profiles/). sort_word
// selects which u64 of the pair carries the digit.
// FUSE_GATHER (AoS only): the writeout copies each pair's whole RECORD
// instead of the pair — the final sort pass IS the gather.
// timing, when set, accumulates the AoS phases' clock ticks.
template <bool HAS_VAL, int IT, bool AOS, int BS = BLOCK,
          bool FUSE_GATHER = false>
__global__ __launch_bounds__(BS) void onesweep_pass_kernel(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
    uint32_t n, int shift, uint64_t* __restrict__ desc /* [nb][ND] */,
    uint32_t* __restrict__ ticket,
    const uint64_t* __restrict__ key_dst, const uint64_t* __restrict__ val_dst,
    uint64_t* __restrict__ timing = nullptr, int sort_word = 0,
    const uint32_t* __restrict__ rec_words = nullptr, /* FUSE_GATHER */
    uint32_t rec_w4 = 0 /* record words; key_dst then holds per-digit
                           RECORD base addresses */,
    const RecSegment* __restrict__ rec_segs = nullptr, /* FUSE_GATHER: */
    uint32_t rec_nsegs = 0 /* record sources (record_src); 0 = contiguous
                              from rec_words */) {
  constexpr int PBITS = 8;
  constexpr int ND = 1 << PBITS;
  extern __shared__ char smem_raw[];
  constexpr int TILE_T = BS * IT;
  constexpr int NWT = BS / kWave;
  using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
  uint64_t* exch = reinterpret_cast<uint64_t*>(smem_raw);  // [TILE_T] or
  u64x2* exch2 = reinterpret_cast<u64x2*>(smem_raw);       // [TILE_T] pairs
  uint32_t* counters = reinterpret_cast<uint32_t*>(
      exch + (AOS ? 2 * TILE_T : TILE_T));
  uint32_t* start = counters + NWT * ND;
  uint32_t* pref = start + ND;
  uint32_t* sums = pref + ND;  // [BS]
  uint32_t* vb_sh = sums + BS;
  uint8_t* dsort = reinterpret_cast<uint8_t*>(vb_sh + 4);  // [TILE_T], !AOS

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  if (tid == 0) *vb_sh = atomicAdd(ticket, 1);
  for (int d = tid; d < NWT * ND; d += BS) counters[d] = 0;
  __syncthreads();
  const uint32_t b = *vb_sh;  // execution-ordered virtual block id
  const uint64_t tile_start = (uint64_t)b * TILE_T;
  const uint32_t tile_n =
      (uint32_t)min((uint64_t)TILE_T, (uint64_t)n - tile_start);
  uint32_t* my = counters + wave * ND;

  uint64_t t0 = timing ? __builtin_amdgcn_s_memrealtime() : 0;
  // phase A: stable per-wave ranks; digit(8b)|rank(16b) packed per elem.
  // Loads run in their own loop FIRST so all IT 16-byte loads are in
  // flight before the serial per-wave LDS counter chain starts — fusing
  // load+rank serialized loads behind LDS RMWs (phase A 11.4 -> 8.2 us
  // per block, full sort 7.56 -> 7.15 ms / 64M).
  uint64_t key_reg[IT];
  uint64_t val_reg[AOS ? IT : 1];
  uint32_t digrank[IT];
  const uint64_t chunk = tile_start + (uint64_t)wave * (IT * kWave);
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    bool valid = e < n;
    if (AOS) {
      u64x2 kv = valid ? reinterpret_cast<const u64x2*>(keys)[e]
                       : u64x2{0, 0};
      key_reg[i] = kv.x;
      val_reg[AOS ? i : 0] = kv.y;
    } else {
      key_reg[i] = valid ? keys[e] : 0;
    }
  }
  // rank in iteration PAIRS: both iterations' per-bit ballots are held
  // in registers, so the pair's ranks and the single LDS counter update
  // per digit need only ONE serial LDS round trip per two iterations —
  // the serial chain was 13% of a pass.
  static_assert(IT % 2 == 0, "pair ranking needs even IT");
  const uint64_t lt = (1ull << lane) - 1;
#pragma unroll
  for (int c = 0; c < IT / 2; ++c) {
    const int i0 = 2 * c, i1 = 2 * c + 1;
    uint64_t e0 = chunk + (uint64_t)i0 * kWave + lane;
    uint64_t e1 = chunk + (uint64_t)i1 * kWave + lane;
    bool val0 = e0 < n, val1 = e1 < n;
    // sort_word selects WHICH u64 of the AoS pair orders this pass
    // (the 80-bit-key path sorts 16 aux bits before the 64 prefix bits)
    uint64_t sk0 = (AOS && sort_word) ? val_reg[AOS ? i0 : 0] : key_reg[i0];
    uint64_t sk1 = (AOS && sort_word) ? val_reg[AOS ? i1 : 0] : key_reg[i1];
    uint32_t d0 = (uint32_t)(sk0 >> shift) & (ND - 1);
    uint32_t d1 = (uint32_t)(sk1 >> shift) & (ND - 1);
    uint64_t vm0 = __ballot(val0), vm1 = __ballot(val1);
    uint64_t v0[PBITS], v1[PBITS];
#pragma unroll
    for (int b = 0; b < PBITS; ++b) v0[b] = __ballot((d0 >> b) & 1);
#pragma unroll
    for (int b = 0; b < PBITS; ++b) v1[b] = __ballot((d1 >> b) & 1);
    // per-chunk bases read BEFORE this chunk's single update round
    uint32_t base0 = val0 ? my[d0] : 0;
    uint32_t base1 = val1 ? my[d1] : 0;
    uint64_t m0 = match_votes<PBITS>(v0, vm0, d0);
    uint64_t m1 = match_votes<PBITS>(v1, vm1, d1);
    uint64_t cross1 = match_votes<PBITS>(v0, vm0, d1);  // i0 elems == d1
    uint32_t r0 = base0 + (uint32_t)__popcll(m0 & lt);
    uint32_t r1 = base1 + (uint32_t)__popcll(cross1)
                  + (uint32_t)__popcll(m1 & lt);
    digrank[i0] = (d0 << 16) | (val0 ? r0 : 0);
    digrank[i1] = (d1 << 16) | (val1 ? r1 : 0);
    // one LDS update per digit per PAIR: the i0 leader of a digit adds
    // both iterations' counts; digits present only in i1 are added by
    // their i1 leader
    if (val0 && (m0 & lt) == 0) {
      uint64_t cross0 = match_votes<PBITS>(v1, vm1, d0);
      my[d0] = base0 + (uint32_t)__popcll(m0) + (uint32_t)__popcll(cross0);
    }
    if (val1 && (m1 & lt) == 0 && cross1 == 0)
      my[d1] = base1 + (uint32_t)__popcll(m1);
  }
  __syncthreads();

  // per-digit wave-exclusive scan + block totals into start[]
  for (int d = tid; d < ND; d += BS) {
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < NWT; ++w) {
      uint32_t t = counters[w * ND + d];
      counters[w * ND + d] = run;
      run += t;
    }
    start[d] = run;
  }
  __syncthreads();

  // publish this block's AGGREGATE as early as possible — consumers'
  // lookbacks are gated on it; our own walk is DEFERRED to overlap the
  // LDS exchange below (the walk is wait-dominated: it costs ~30% of the
  // pass when run serially here — profiles/r01)
  uint64_t my_total = 0;
  if (tid < ND) {
    my_total = start[tid];
    uint64_t* slot = &desc[(uint64_t)b * ND + tid];
    if (b == 0) {
      __hip_atomic_store(slot, FLAG_INC | my_total, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      pref[tid] = 0;
    } else {
      __hip_atomic_store(slot, FLAG_AGG | my_total, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // block-local digit starts (exclusive scan of totals)
  block_exscan<BS>(start, sums, ND);  // includes the needed __syncthreads

  uint64_t t1 = timing ? __builtin_amdgcn_s_memrealtime() : 0;
  if (AOS) {
    // pair exchange first: the deferred lookback's wait overlaps it
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      uint64_t e = chunk + (uint64_t)i * kWave + lane;
      if (e < n) {
        uint32_t d = digrank[i] >> 16;
        uint32_t j = start[d] + my[d] + (digrank[i] & 0xFFFF);
        exch2[j] = u64x2{key_reg[i], val_reg[AOS ? i : 0]};
      }
    }
    uint64_t t2 = timing ? __builtin_amdgcn_s_memrealtime() : 0;
    if (b != 0 && tid < ND) lookback_walk<ND>(desc, b, tid, my_total, pref);
    __syncthreads();
    uint64_t t3 = timing ? __builtin_amdgcn_s_memrealtime() : 0;
    if (FUSE_GATHER) {
      // copy each slot's RECORD to its final position: key_dst[d]
      // holds per-digit record bases. Each slot's pair is replaced IN
      // PLACE by its (record source, destination) addresses — digit,
      // offset and index derived once per slot — then the block runs
      // the same batched word copy as gather_records (writes coalesce
      // within digit runs, reads are the random per-record chunks the
      // separate gather paid anyway). Block-uniform code: every thread
      // reaches the barrier.
      GatherSlot* slots = reinterpret_cast<GatherSlot*>(smem_raw);
      for (uint32_t j = tid; j < tile_n; j += BS) {
        u64x2 kv = exch2[j];
        uint32_t d = (uint32_t)((uint64_t)(sort_word ? kv.y : kv.x)
                                >> shift) & (ND - 1);
        uint32_t off = pref[d] + (j - start[d]);
        uint64_t idx = (uint64_t)kv.y & AUX_IDX_MASK;
        slots[j] = GatherSlot{
            record_src(rec_words, rec_segs, rec_nsegs, idx, rec_w4),
            reinterpret_cast<uint32_t*>(key_dst[d]) +
                (uint64_t)off * rec_w4};
      }
      __syncthreads();
      copy_record_words<BS, GATHER_BATCH>(slots, tile_n, rec_w4);
    } else {
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        uint32_t j = (uint32_t)i * BS + tid;
        if (j < tile_n) {
          u64x2 kv = exch2[j];
          uint32_t d = (uint32_t)((uint64_t)(sort_word ? kv.y : kv.x)
                                  >> shift) & (ND - 1);
          uint32_t off = pref[d] + (j - start[d]);
          reinterpret_cast<u64x2*>(key_dst[d])[off] = kv;
        }
      }
    }
    if (timing && tid == 0) {
      uint64_t t4 = __builtin_amdgcn_s_memrealtime();
      atomicAdd(&timing[0], t1 - t0);  // phase A (+scans+publish)
      atomicAdd(&timing[1], t2 - t1);  // exchange
      atomicAdd(&timing[2], t3 - t2);  // lookback walk + barrier
      atomicAdd(&timing[3], t4 - t3);  // writeout
    }
    return;
  }
  if (b != 0 && tid < ND) lookback_walk<ND>(desc, b, tid, my_total, pref);

  // SoA path: key exchange + write-out, then val exchange + write-out
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    uint64_t e = chunk + (uint64_t)i * kWave + lane;
    if (e < n) {
      uint32_t d = digrank[i] >> 16;
      uint32_t j = start[d] + my[d] + (digrank[i] & 0xFFFF);
      digrank[i] = j;  // reuse: local sorted position
      exch[j] = key_reg[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    uint32_t j = i * BS + tid;
    if (j < tile_n) {
      uint64_t k = exch[j];
      uint32_t d = (uint32_t)(k >> shift) & (ND - 1);
      uint32_t off = pref[d] + (j - start[d]);
      dsort[j] = (uint8_t)d;
      reinterpret_cast<uint64_t*>(key_dst[d])[off] = k;
    }
  }
  if (HAS_VAL) {
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < IT; ++i) {
      uint64_t e = chunk + (uint64_t)i * kWave + lane;
      if (e < n) exch[digrank[i]] = vals[e];
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < IT; ++i) {
      uint32_t j = i * BS + tid;
      if (j < tile_n) {
        uint32_t d = dsort[j];
        uint32_t off = pref[d] + (j - start[d]);
        reinterpret_cast<uint64_t*>(val_dst[d])[off] = exch[j];
      }
    }
  }
}

// digit bases for pass p from the all-pass totals; rec_bytes = 8 (SoA)
// or 16 (AoS interleaved records)
template <int ND = 256>
__global__ void onesweep_digit_bases_kernel(
    const uint32_t* __restrict__ totals /* [pass][ND] */, int pass,
    uint64_t out_keys, uint64_t out_vals, uint64_t* __restrict__ key_dst,
    uint64_t* __restrict__ val_dst, int rec_bytes) {
  __shared__ uint32_t arr[ND];
  __shared__ uint32_t sums[BLOCK];
  const int tid = threadIdx.x;
  if (tid < ND) arr[tid] = totals[pass * ND + tid];
  __syncthreads();
  block_exscan(arr, sums, ND);
  if (tid < ND) {
    key_dst[tid] = out_keys + (uint64_t)arr[tid] * rec_bytes;
    val_dst[tid] = out_vals ? out_vals + (uint64_t)arr[tid] * rec_bytes : 0;
  }
}

// ---------------------------------------------------------------------------
// Wide-record machinery (VERDICT r01 missing item 3: the reference serves
// WHATEVER bytes the writer produced — RdmaMappedFile.java:113-157 —
// while the r01 fast path handled only 16-byte records; canonical
// TeraSort is 10 B key + 90 B value = 100 B records).
//
// Design: records stay put while 16-byte (sortkey, aux) PAIRS flow
// through the existing radix machinery, and each W-byte record moves
// once, to its final position:
//   * extract_pairs: record -> (key-prefix u64, aux = keylo16<<48 | idx);
//     on the map side pair.x is the record's PARTITION ID instead
//   * sort (reduce side): LSD passes over the pairs (`sort_word` selects
//     which u64 of the pair the digit comes from, so the 80-bit key sorts
//     as 16 aux bits then 64 prefix bits, LSD-stable); the FINAL pass
//     writes the records instead of the pairs (FUSE_GATHER)
//   * partition (map side), up to 256 partitions: count the ids
//     (count_pair_digits) so the host can lay out the HBM blocks, then
//     that same fused pass, once, with the block addresses as its
//     per-digit bases (partition_records_fused). No grouped copy of the
//     pairs and no separate gather; the pairs enter in input order, so a
//     tile's record reads cover one contiguous span of the source
//   * partition, 257..4096 partitions: hist -> scan -> radix_scatter
//     groups the pairs, gather_records (dst_mode 1) then walks the grouped
//     pairs linearly and copies record idx to its slot — writes are linear
//     (W-byte runs), reads are W-byte contiguous chunks. More than 4096:
//     the same after a two-level grouping of the pairs by partition id
// Both sides move each record exactly once.
// Traffic: ~2.2x the record bytes + ~64 B/pass for the 16 B pairs —
// pair passes cost 16% of what full-record passes would at W = 100.
// extract_pairs itself re-reads practically every 128-byte line of its
// input at W = 100 (10 key bytes per 100-byte record), i.e. one more
// pass over the records. The map side needs that pass (the gather cannot
// place a record before its pair exists); the reduce side does not: its
// one-sided fetch moves every record through registers anyway, and
// fetch_records_kernel emits the pairs from there.
// Nor does the reduce side need the records in one buffer: a pair's aux
// index is a position in the reader's VIRTUAL arena, and both consumers of
// it — gather_records_kernel and the fused final sort pass — find the
// record through record_src, a segment table of (first index, address)
// runs. So blocks this executor owns are not fetched at all: the
// extract-only variant of fetch_records_kernel reads them once for the
// pairs and the final pass gathers them from the shuffle's blocks, the
// same random W-byte reads over the same span it paid on the arena copy
// (profiles/r08_inplace_local_records.md). Each local record is then
// moved twice, map write and final pass, not three times.

// Key layout inside a record: bytes [0,8) u64 LE prefix, bytes [8,10)
// u16 LE low bits (key_bytes == 8 or 10); 80-bit order = (prefix, lo).
// pid_func >= 0: pair.x carries the PARTITION ID of the record instead
// of the raw prefix — the two-level >4096-partition path then radixes
// the pid itself (coarse bits then fine bits).
__global__ __launch_bounds__(BLOCK) void extract_pairs_kernel(
    const uint8_t* __restrict__ recs, uint64_t n, uint32_t rec_bytes,
    uint32_t key_bytes, uint64_t* __restrict__ pairs, int pid_func,
    int pid_shift, uint32_t pid_mask, uint32_t pid_nparts,
    uint64_t idx_base /* aux indices are idx_base + e: per-chunk extracts
                         reference records in a larger arena */) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < n;
       e += stride) {
    const uint8_t* p = recs + e * rec_bytes;
    // 4-byte-aligned loads (rec_bytes % 4 == 0 enforced host-side)
    uint32_t lo = *reinterpret_cast<const uint32_t*>(p);
    uint32_t hi = *reinterpret_cast<const uint32_t*>(p + 4);
    uint64_t prefix = ((uint64_t)hi << 32) | lo;
    uint64_t aux = idx_base + e;
    if (key_bytes > 8) {
      uint16_t klo = (uint16_t)(*reinterpret_cast<const uint32_t*>(p + 8));
      aux |= (uint64_t)klo << 48;
    }
    uint64_t x = pid_func < 0
        ? prefix
        : (uint64_t)digit_of(prefix, pid_shift, pid_mask, pid_func,
                             pid_nparts);
    reinterpret_cast<ulonglong2*>(pairs)[e] = ulonglong2{x, aux};
  }
}

// Move records to their final slots following the grouped/sorted pairs.
// Slot j's record index comes from pairs[2j+1]; its destination is
//   dst_mode 0: out_base + j*rec_bytes                  (sorted output)
//   dst_mode 1: dst_addr[d] + (j - dstart[d])*rec_bytes (partition path,
//               d = digit_of(pairs[2j]) — per-digit HBM block positions)
//
// The copy is latency-bound unless many record bytes are in flight per
// CU (random ~100-byte reads from a buffer far past the Infinity Cache),
// so the block first stages every record's (source, destination) address
// pair in LDS from coalesced 16-byte pair loads — no global load sits in
// front of a record load, and index / digit / destination are derived
// once per record — and then copies in batches: GATHER_BATCH independent
// loads per lane are issued before the first dependent store.
// In flight per CU = resident lanes x GATHER_BATCH x 4 B: 64 KB for the
// stand-alone gather at 8 blocks/CU (48 VGPRs), 32 KB for the fused sort
// pass at 2 x 512 threads. A 16-deep batch measured no faster in either
// kernel and costs the fused pass its second resident block (160 VGPRs)
// — profiles/r03_record_movement.md.
constexpr uint32_t GATHER_MAX_RECS = 1024;  // per block: 16 KB of LDS slots

__global__ __launch_bounds__(BLOCK) void gather_records_kernel(
    const uint32_t* __restrict__ recs, const uint64_t* __restrict__ pairs,
    uint64_t n, uint32_t w4 /* rec_bytes/4 */,
    uint32_t recs_per_block /* <= GATHER_MAX_RECS */, int dst_mode,
    uint64_t out_base, const uint64_t* __restrict__ dst_addr,
    const uint32_t* __restrict__ dstart, int shift, uint32_t mask,
    int func, uint32_t nparts, const RecSegment* __restrict__ segs,
    uint32_t nsegs /* record sources (record_src); 0 = contiguous */) {
  __shared__ GatherSlot slots[GATHER_MAX_RECS];
  const uint64_t r0 = (uint64_t)blockIdx.x * recs_per_block;
  if (r0 >= n) return;
  const uint32_t nr = (uint32_t)min((uint64_t)recs_per_block, n - r0);
  for (uint32_t r = threadIdx.x; r < nr; r += BLOCK) {
    const uint64_t j = r0 + r;
    ulonglong2 pr = reinterpret_cast<const ulonglong2*>(pairs)[j];
    const uint64_t idx = pr.y & AUX_IDX_MASK;
    uint32_t* dst;
    if (dst_mode == 0) {
      dst = reinterpret_cast<uint32_t*>(out_base) + j * w4;
    } else {
      uint32_t d = digit_of(pr.x, shift, mask, func, nparts);
      dst = reinterpret_cast<uint32_t*>(dst_addr[d]) +
            (uint64_t)(uint32_t)(j - dstart[d]) * w4;
    }
    slots[r] = GatherSlot{record_src(recs, segs, nsegs, idx, w4), dst};
  }
  __syncthreads();
  copy_record_words<BLOCK, GATHER_BATCH>(slots, nr, w4);
}

void extract_pairs(uintptr_t recs, uint64_t n, uint32_t rec_bytes,
                   uint32_t key_bytes, uintptr_t pairs, uintptr_t stream,
                   int pid_func, int pid_shift, uint32_t pid_mask,
                   uint32_t pid_nparts, uint64_t idx_base) {
  if (rec_bytes % 4 || rec_bytes < 8)
    throw std::runtime_error("rec_bytes must be a multiple of 4, >= 8");
  if (key_bytes != 8 && key_bytes != 10)
    throw std::runtime_error("key_bytes must be 8 or 10");
  if (n >> 48)
    throw std::runtime_error("record count exceeds 2^48");
  auto s = reinterpret_cast<hipStream_t>(stream);
  uint32_t grid = (uint32_t)min((n + BLOCK - 1) / BLOCK, (uint64_t)4096);
  if ((idx_base + n) >> 48)
    throw std::runtime_error("idx_base + n exceeds 2^48");
  hipLaunchKernelGGL(extract_pairs_kernel, dim3(grid ? grid : 1),
                     dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint8_t*>(recs), n, rec_bytes,
                     key_bytes, reinterpret_cast<uint64_t*>(pairs),
                     pid_func, pid_shift, pid_mask, pid_nparts, idx_base);
  HIP_CHECK(hipGetLastError());
}

void gather_records(uintptr_t recs, uintptr_t pairs, uint64_t n,
                    uint32_t rec_bytes, int dst_mode, uint64_t out_base,
                    uintptr_t dst_addr, uintptr_t dstart, int shift,
                    uint32_t mask, int func, uint32_t nparts,
                    uintptr_t stream, uintptr_t segs, uint32_t nsegs) {
  if (rec_bytes % 4) throw std::runtime_error("rec_bytes % 4 != 0");
  if (nsegs && !segs) throw std::runtime_error("nsegs without a table");
  auto s = reinterpret_cast<hipStream_t>(stream);
  uint32_t w4 = rec_bytes / 4;
  // ~32k words per block (whole copy batches at W = 100 and 256), at
  // most GATHER_MAX_RECS records (the kernel's LDS slot table)
  uint32_t rpb = 32768 / w4;
  if (rpb > GATHER_MAX_RECS) rpb = GATHER_MAX_RECS;
  if (rpb < 1) rpb = 1;
  uint64_t grid = (n + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) throw std::runtime_error("grid too large");
  hipLaunchKernelGGL(gather_records_kernel, dim3((uint32_t)(grid ? grid : 1)),
                     dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint32_t*>(recs),
                     reinterpret_cast<const uint64_t*>(pairs), n, w4, rpb,
                     dst_mode, out_base,
                     reinterpret_cast<const uint64_t*>(dst_addr),
                     reinterpret_cast<const uint32_t*>(dstart), shift, mask,
                     func, nparts, reinterpret_cast<const RecSegment*>(segs),
                     nsegs);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Fused one-sided fetch of wide records: copy a run of n whole W-byte
// records src -> dst AND emit every record's (prefix, aux) pair, exactly
// what extract_pairs_kernel writes for pid_func < 0. The reduce side used
// to copy the run (hipMemcpyAsync) and then read practically every line of
// the arena again to pick 10 key bytes out of each 100-byte record; here
// the key words are taken from the registers that move them.
//
// A block owns a tile of whole records, which is one contiguous word range
// on both sides, and moves it one dword per lane (src and dst are only
// 4-byte aligned, independently of each other), U independent loads per
// lane before the first store as in copy_record_words. Word q of the tile
// is word q % w4 of record q / w4, tracked with the same block-uniform
// (BS / w4, BS % w4) stepping; a lane holding word 0, 1 or 2 of a record
// also drops it into the LDS key table. After one barrier, one thread per
// record assembles the pair and the block stores the pairs as coalesced
// 16-byte stores.
//
// INVARIANT: every word of [src, src + n * w4) is loaded exactly once and
// nothing outside it is touched — lanes past the end of the last tile load
// nothing — so the kernel is equally valid for a peer-mapped source. dst
// gets exactly [dst, dst + n * w4), pairs exactly [pairs, pairs + 2n).
//
// COPY = false is the in-place variant (extract_records): the same loads
// and key-table writes, no record store, dst never touched. The reader uses
// it for blocks this executor owns — copying them from one place in its
// HBM to another buys nothing, the sort gathers them from where they are
// (record_src) — and the fetch then moves 0.54x the bytes.
//
// Tile: about 4096 words (16 KB, two batches) per block. With src and dst
// 4 and 12 bytes off a 16-byte boundary, 4 GB of 100-byte records moved at
// 4.5-4.7 TB/s (records read + written + pairs written) with 1024-record
// tiles and at 5.25-5.55 TB/s with 128..256-record tiles, against 5.6 TB/s
// for either with both sides 16-byte aligned; 16 bytes per lane at 4-byte
// alignment (the tile is one contiguous range, so there is no per-record
// tail) was no faster than one dword per lane at these tile sizes
// (profiles/r06_fused_fetch.md).
constexpr uint32_t FETCH_MAX_RECS = 1024;  // per block: 12 KB key table
constexpr uint32_t FETCH_BLOCK_WORDS = 4096;
constexpr int FETCH_BATCH = GATHER_BATCH;

static inline uint32_t fetch_block_records_w4(uint32_t w4) {
  uint32_t rpb = FETCH_BLOCK_WORDS / w4;
  if (rpb > FETCH_MAX_RECS) rpb = FETCH_MAX_RECS;
  return rpb < 1 ? 1 : rpb;
}

// One batch of the tile: U words per lane, loads first. WHOLE (every lane
// has all U words) is decided per batch for the whole block and compiled
// as its own body, so neither the loads nor the stores of a whole batch
// sit behind a per-lane test or a wait that only the tile's last batch
// needs. (r, o) = record and word-in-record of the lane's next word.
template <int BS, int U, bool WHOLE, bool COPY>
__device__ __forceinline__ void fetch_batch(
    const uint32_t* __restrict__ s, uint32_t* __restrict__ d,
    uint32_t* keytab, uint32_t q0, uint32_t total, uint32_t w4, uint32_t dr,
    uint32_t dc, uint32_t& r, uint32_t& o) {
  uint32_t v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t q = q0 + (uint32_t)u * BS + threadIdx.x;
    v[u] = (WHOLE || q < total) ? s[q] : 0u;
  }
  // without the store only words 0..2 of a record are used, and the
  // compiler would sink some of the loads behind that per-lane test: keep
  // the batch what it is with COPY, U unconditional loads up front (an
  // empty statement per value, after ALL loads are issued)
  if (!COPY) {
#pragma unroll
    for (int u = 0; u < U; ++u) asm volatile("" : "+v"(v[u]));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t q = q0 + (uint32_t)u * BS + threadIdx.x;
    if (WHOLE || q < total) {
      if (COPY) d[q] = v[u];
      if (o < 3) keytab[r * 3 + o] = v[u];
    }
    o += dc;
    r += dr;
    if (o >= w4) {
      o -= w4;
      ++r;
    }
  }
}

template <int BS, int U, bool COPY>
__global__ __launch_bounds__(BS) void fetch_records_kernel(
    const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t n,
    uint32_t w4 /* rec_bytes/4 */,
    uint32_t recs_per_block /* <= FETCH_MAX_RECS */, uint32_t key_bytes,
    uint64_t* __restrict__ pairs, uint64_t idx_base) {
  __shared__ uint32_t keytab[FETCH_MAX_RECS * 3];  // words 0..2 per record
  const uint64_t r0 = (uint64_t)blockIdx.x * recs_per_block;
  if (r0 >= n) return;
  const uint32_t nr = (uint32_t)min((uint64_t)recs_per_block, n - r0);
  const uint32_t total = nr * w4;
  const uint32_t* __restrict__ s = src + r0 * w4;
  uint32_t* __restrict__ d = COPY ? dst + r0 * w4 : nullptr;
  const uint32_t tid = threadIdx.x;
  const uint32_t dr = BS / w4, dc = BS % w4;
  uint32_t r = tid / w4, o = tid % w4;
  const uint32_t whole_end = total - total % (BS * U);
  uint32_t q0 = 0;
#pragma unroll 1
  for (; q0 < whole_end; q0 += BS * U)
    fetch_batch<BS, U, true, COPY>(s, d, keytab, q0, total, w4, dr, dc, r,
                                   o);
  if (q0 < total)
    fetch_batch<BS, U, false, COPY>(s, d, keytab, q0, total, w4, dr, dc, r,
                                    o);
  __syncthreads();
  for (uint32_t j = tid; j < nr; j += BS) {
    const uint64_t prefix =
        ((uint64_t)keytab[j * 3 + 1] << 32) | keytab[j * 3];
    uint64_t aux = idx_base + r0 + j;
    // word 2 exists whenever key_bytes > 8 (rec_bytes >= 12 host-side)
    if (key_bytes > 8) aux |= (uint64_t)(uint16_t)keytab[j * 3 + 2] << 48;
    reinterpret_cast<ulonglong2*>(pairs)[r0 + j] = ulonglong2{prefix, aux};
  }
}

uint32_t fetch_block_records(uint32_t rec_bytes) {
  if (rec_bytes % 4 || rec_bytes < 8)
    throw std::runtime_error("rec_bytes must be a multiple of 4, >= 8");
  return fetch_block_records_w4(rec_bytes / 4);
}

void fetch_records(uintptr_t dst, uintptr_t src, uint64_t n,
                   uint32_t rec_bytes, uint32_t key_bytes, uintptr_t pairs,
                   uint64_t idx_base, uintptr_t stream) {
  if (rec_bytes % 4 || rec_bytes < 8)
    throw std::runtime_error("rec_bytes must be a multiple of 4, >= 8");
  if (key_bytes != 8 && key_bytes != 10)
    throw std::runtime_error("key_bytes must be 8 or 10");
  if (key_bytes > 8 && rec_bytes < 12)
    throw std::runtime_error("key_bytes 10 needs rec_bytes >= 12");
  if ((n >> 48) || ((idx_base + n) >> 48))
    throw std::runtime_error("idx_base + n exceeds 2^48");
  if ((src | dst) % 4 || pairs % 16)
    throw std::runtime_error(
        "fetch_records: src/dst need 4-byte, pairs 16-byte alignment");
  if (n == 0) return;
  const uint32_t w4 = rec_bytes / 4;
  const uint32_t rpb = fetch_block_records_w4(w4);
  const uint64_t grid = (n + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) throw std::runtime_error("grid too large");
  hipLaunchKernelGGL((fetch_records_kernel<BLOCK, FETCH_BATCH, true>),
                     dim3((uint32_t)grid), dim3(BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t*>(src),
                     reinterpret_cast<uint32_t*>(dst), n, w4, rpb, key_bytes,
                     reinterpret_cast<uint64_t*>(pairs), idx_base);
  HIP_CHECK(hipGetLastError());
}

// The in-place variant: the same loads and the same key-table writes, no
// record store — the records stay where they are (a block of this
// executor's own shuffle output) and the sort gathers them from there
// through a segment table (record_src). One streaming read of the run.
void extract_records(uintptr_t src, uint64_t n, uint32_t rec_bytes,
                     uint32_t key_bytes, uintptr_t pairs, uint64_t idx_base,
                     uintptr_t stream) {
  if (rec_bytes % 4 || rec_bytes < 8)
    throw std::runtime_error("rec_bytes must be a multiple of 4, >= 8");
  if (key_bytes != 8 && key_bytes != 10)
    throw std::runtime_error("key_bytes must be 8 or 10");
  if (key_bytes > 8 && rec_bytes < 12)
    throw std::runtime_error("key_bytes 10 needs rec_bytes >= 12");
  if ((n >> 48) || ((idx_base + n) >> 48))
    throw std::runtime_error("idx_base + n exceeds 2^48");
  if (src % 4 || pairs % 16)
    throw std::runtime_error(
        "extract_records: src needs 4-byte, pairs 16-byte alignment");
  if (n == 0) return;
  const uint32_t w4 = rec_bytes / 4;
  const uint32_t rpb = fetch_block_records_w4(w4);
  const uint64_t grid = (n + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) throw std::runtime_error("grid too large");
  hipLaunchKernelGGL((fetch_records_kernel<BLOCK, FETCH_BATCH, false>),
                     dim3((uint32_t)grid), dim3(BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint32_t*>(src),
                     static_cast<uint32_t*>(nullptr), n, w4, rpb, key_bytes,
                     reinterpret_cast<uint64_t*>(pairs), idx_base);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Tie repair for the truncated wide-record sort (sort_records_u64 below).
// The pairs arrive stably ordered by the RUN BITS only — prefix
// bits [lo_bit, top), selected by run_mask — so elements that agree on
// them are adjacent and in input order. With 2^run_bits >= 8n such runs
// are rare and short for non-degenerate keys, and ordering each of them
// by (prefix & lo_mask, aux) as one 128-bit value gives exactly what the
// skipped low LSD passes would have: aux = keylo16 << 48 | idx, so that
// order IS the remaining key bits with ties broken by input index. Bits
// at and above `top` are deliberately ignored — the stable final pass
// sorts by them afterwards.
//
// A run belongs to the block whose own tile holds its first element; the
// owner insertion-sorts runs of 2..TIE_L elements in LDS (one thread per
// run, runs are disjoint) and writes back only runs it changed. A run
// longer than TIE_L is left alone and reported through *flag, and the host
// then falls back to the full LSD sequence. No cross-block communication.
constexpr int TIE_BS = 256;
constexpr int TIE_IT = 8;
constexpr int TIE_TILE = TIE_BS * TIE_IT;  // 2048 pairs, 32 KB of LDS
constexpr int TIE_L = 32;                  // longest run repaired in place

__global__ __launch_bounds__(TIE_BS) void tie_repair_kernel(
    uint64_t* pairs, uint32_t n, uint64_t run_mask, uint64_t lo_mask,
    uint32_t* __restrict__ flag) {
  using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
  // sh[j] = element base + j: the tile, then TIE_L halo elements — the
  // TIE_L - 1 a run starting at the tile's last element may cover, plus
  // the one whose run bits tell whether that run is longer still
  __shared__ u64x2 sh[TIE_TILE + TIE_L];
  __shared__ uint64_t pred_sh;
  u64x2* g = reinterpret_cast<u64x2*>(pairs);
  const int tid = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * TIE_TILE;
  const uint32_t avail =  // elements of sh that exist (base < n always)
      (uint32_t)min((uint64_t)(TIE_TILE + TIE_L), (uint64_t)n - base);
  const uint32_t tile_n = min(avail, (uint32_t)TIE_TILE);
  // IN PLACE: the predecessor and the halo belong to neighbouring blocks,
  // which may be rewriting them while they are read here. That is benign
  // only because every value that can ever stand in such a slot is a
  // member of the same run, i.e. has the same run bits, and run bits are
  // all this block ever uses of an element it does not own (halo elements
  // of a run that STARTS in this tile are owned here and written by no
  // one else).
  if (tile_n == TIE_TILE) {  // full tile: all loads issued before any use
    u64x2 v[TIE_IT];
#pragma unroll
    for (int k = 0; k < TIE_IT; ++k) v[k] = g[base + k * TIE_BS + tid];
#pragma unroll
    for (int k = 0; k < TIE_IT; ++k) sh[k * TIE_BS + tid] = v[k];
    if (tid < TIE_L && TIE_TILE + tid < avail)
      sh[TIE_TILE + tid] = g[base + TIE_TILE + tid];
  } else {
    for (uint32_t j = tid; j < tile_n; j += TIE_BS) sh[j] = g[base + j];
  }
  if (tid == TIE_L && base > 0) pred_sh = pairs[2 * (base - 1)];
  __syncthreads();

#pragma unroll 1
  for (uint32_t i = tid; i < tile_n; i += TIE_BS) {
    const uint64_t k = sh[i].x;
    const bool start =
        i ? ((sh[i - 1].x ^ k) & run_mask) != 0
          : (base == 0 || ((pred_sh ^ k) & run_mask) != 0);
    if (!start || i + 1 >= avail || ((sh[i + 1].x ^ k) & run_mask)) continue;
    // a run of >= 2 starts here; i + TIE_L < TILE + TIE_L bounds the scan
    const uint32_t lim = min(avail - i, (uint32_t)TIE_L + 1);
    uint32_t len = 2;
#pragma unroll 1
    while (len < lim && ((sh[i + len].x ^ k) & run_mask) == 0) ++len;
    if (len > TIE_L) {
      atomicOr(flag, 1u);
      continue;
    }
    bool changed = false;
#pragma unroll 1
    for (uint32_t a = 1; a < len; ++a) {
      const u64x2 x = sh[i + a];
      const uint64_t xk = x.x & lo_mask;
      uint32_t b = a;
      while (b > 0) {
        const u64x2 u = sh[i + b - 1];
        const uint64_t uk = u.x & lo_mask;
        if (uk < xk || (uk == xk && u.y <= x.y)) break;
        sh[i + b] = u;
        --b;
      }
      if (b != a) {
        sh[i + b] = x;
        changed = true;
      }
    }
    if (changed)
#pragma unroll 1
      for (uint32_t a = 0; a < len; ++a) g[base + i + a] = sh[i + a];
  }
}

// ---------------------------------------------------------------------------
// Microbench probe: emulate the scatter's write pattern — each block
// writes its tile as `nregions` bursts of `burst` bytes at region-strided
// scattered offsets. Measures HBM efficiency vs burst length to size the
// optimization headroom (not part of the data path).

__global__ __launch_bounds__(BLOCK) void probe_scatter_write_kernel(
    uint64_t* __restrict__ out, uint64_t region_elems, uint32_t nregions,
    uint32_t burst_elems, uint32_t bursts_per_block) {
  // block b writes bursts_per_block bursts; burst i goes to region
  // (b*7 + i) % nregions at offset (b * bursts_per_block + i) scaled —
  // scattered across regions like the radix scatter's digit streams.
  const uint32_t b = blockIdx.x;
  for (uint32_t i = 0; i < bursts_per_block; ++i) {
    uint32_t region = (b * 7u + i) % nregions;
    uint64_t off_in_region =
        ((uint64_t)(b * 1315423911u + i * 2654435761u)) %
        (region_elems - burst_elems);
    uint64_t* dst = out + (uint64_t)region * region_elems + off_in_region;
    for (uint32_t e = threadIdx.x; e < burst_elems; e += BLOCK)
      dst[e] = (uint64_t)b * i + e;
  }
}

void probe_scatter_write(uintptr_t out, uint64_t region_elems,
                         uint32_t nregions, uint32_t burst_elems,
                         uint32_t bursts_per_block, uint32_t grid,
                         uintptr_t stream) {
  hipLaunchKernelGGL(probe_scatter_write_kernel, dim3(grid), dim3(BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<uint64_t*>(out), region_elems, nregions,
                     burst_elems, bursts_per_block);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Sort-merge join (merge kernel for SQL sort-merge join).
// Both sides radix-sorted first; the merge is per-A-row binary search in
// sorted B (log nb coherent loads — neighbouring threads probe
// neighbouring B ranges, so the walk stays in L2), then pair emission at
// scanned offsets.

__device__ __forceinline__ uint32_t lower_bound_u64(
    const uint64_t* __restrict__ arr, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (arr[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void join_count_kernel(
    const uint64_t* __restrict__ a_keys, uint32_t na,
    const uint64_t* __restrict__ b_keys, uint32_t nb_,
    uint32_t* __restrict__ counts, uint32_t* __restrict__ lo_idx) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < na;
       i += stride) {
    uint64_t k = a_keys[i];
    uint32_t lo = lower_bound_u64(b_keys, nb_, k);
    uint32_t hi = lo;
    while (hi < nb_ && b_keys[hi] == k) ++hi;  // runs are short for ~unique keys
    counts[i] = hi - lo;
    lo_idx[i] = lo;
  }
}

__global__ __launch_bounds__(BLOCK) void join_emit_kernel(
    const uint64_t* __restrict__ a_keys, const uint64_t* __restrict__ a_vals,
    uint32_t na, const uint64_t* __restrict__ b_vals,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ lo_idx,
    const uint64_t* __restrict__ offsets,
    uint64_t* __restrict__ out_key, uint64_t* __restrict__ out_a,
    uint64_t* __restrict__ out_b) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < na;
       i += stride) {
    uint32_t cnt = counts[i];
    if (!cnt) continue;
    uint64_t off = offsets[i];
    uint32_t lo = lo_idx[i];
    uint64_t k = a_keys[i];
    uint64_t av = a_vals ? a_vals[i] : 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (out_key) out_key[off + j] = k;
      if (out_a) out_a[off + j] = av;
      out_b[off + j] = b_vals[lo + j];
    }
  }
}

static inline uint32_t join_grid(uint32_t n) {
  uint32_t g = (n + BLOCK - 1) / BLOCK;
  return g > 2048 ? 2048 : (g ? g : 1);
}

void join_count(uintptr_t a_keys, uint32_t na, uintptr_t b_keys, uint32_t nb_,
                uintptr_t counts, uintptr_t lo_idx, uintptr_t stream) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(join_count_kernel, dim3(join_grid(na)), dim3(BLOCK), 0,
                     s, reinterpret_cast<const uint64_t*>(a_keys), na,
                     reinterpret_cast<const uint64_t*>(b_keys), nb_,
                     reinterpret_cast<uint32_t*>(counts),
                     reinterpret_cast<uint32_t*>(lo_idx));
  HIP_CHECK(hipGetLastError());
}

void join_emit(uintptr_t a_keys, uintptr_t a_vals, uint32_t na,
               uintptr_t b_vals, uintptr_t counts, uintptr_t lo_idx,
               uintptr_t offsets, uintptr_t out_key, uintptr_t out_a,
               uintptr_t out_b, uintptr_t stream) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(join_emit_kernel, dim3(join_grid(na)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint64_t*>(a_keys),
                     reinterpret_cast<const uint64_t*>(a_vals), na,
                     reinterpret_cast<const uint64_t*>(b_vals),
                     reinterpret_cast<const uint32_t*>(counts),
                     reinterpret_cast<const uint32_t*>(lo_idx),
                     reinterpret_cast<const uint64_t*>(offsets),
                     reinterpret_cast<uint64_t*>(out_key),
                     reinterpret_cast<uint64_t*>(out_a),
                     reinterpret_cast<uint64_t*>(out_b));
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// host wrappers

static inline uint32_t num_tiles(uint32_t n) {
  return (uint32_t)(((uint64_t)n + TILE - 1) / TILE);
}

size_t radix_hist_bytes(uint32_t n, int nbits) {
  return (size_t)(1u << nbits) * num_tiles(n) * sizeof(uint32_t);
}

template <int NBITS>
static void hist_launch(const uint64_t* keys, uint32_t n, int shift,
                        uint32_t* hist, hipStream_t s, int func = 0,
                        int in_stride = 1, uint32_t nparts = 0) {
  uint32_t nb = num_tiles(n);
  size_t lds = (size_t)NW * (1 << NBITS) * 4;
  hipLaunchKernelGGL(radix_hist_kernel<NBITS>, dim3(nb), dim3(BLOCK), lds, s,
                     keys, n, shift, hist, nb, func, in_stride, nparts);
  HIP_CHECK(hipGetLastError());
}

template <int NBITS, bool HAS_VAL>
static void scatter_launch(const uint64_t* keys, const uint64_t* vals,
                           uint32_t n, int shift, const uint32_t* hist,
                           const uint64_t* key_dst, const uint64_t* val_dst,
                           hipStream_t s, int func = 0, int aos_out = 0,
                           int in_stride = 1, uint32_t nparts = 0) {
  constexpr int ND = 1 << NBITS;
  uint32_t nb = num_tiles(n);
  size_t lds = (size_t)TILE * 8 + (size_t)NW * ND * 4 + (size_t)ND * 4 * 2 +
               BLOCK * 4;
  auto kfn = radix_scatter_kernel<NBITS, HAS_VAL>;
  // one flag per <NBITS, HAS_VAL>: the keys+vals and keys-only kernels
  // are different functions, each needs the attribute set on itself
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(kfn),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  hipLaunchKernelGGL(kfn, dim3(nb), dim3(BLOCK), lds, s, keys, vals, n, shift,
                     hist, nb, key_dst, val_dst, func, aos_out, in_stride,
                     nparts);
  HIP_CHECK(hipGetLastError());
}

#define DISPATCH_NBITS(nbits, FN, ...)                        \
  switch (nbits) {                                            \
    case 4: FN<4>(__VA_ARGS__); break;                        \
    case 5: FN<5>(__VA_ARGS__); break;                        \
    case 6: FN<6>(__VA_ARGS__); break;                        \
    case 7: FN<7>(__VA_ARGS__); break;                        \
    case 8: FN<8>(__VA_ARGS__); break;                        \
    case 9: FN<9>(__VA_ARGS__); break;                        \
    case 10: FN<10>(__VA_ARGS__); break;                      \
    case 11: FN<11>(__VA_ARGS__); break;                      \
    case 12: FN<12>(__VA_ARGS__); break;                      \
    default: throw std::runtime_error("nbits must be 4..12"); \
  }

void radix_hist(uintptr_t keys, uint32_t n, int shift, int nbits,
                uintptr_t hist, uintptr_t stream, int func, int in_stride,
                uint32_t nparts) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_NBITS(nbits, hist_launch, reinterpret_cast<const uint64_t*>(keys),
                 n, shift, reinterpret_cast<uint32_t*>(hist), s, func,
                 in_stride, nparts);
}

size_t radix_scan_ws_bytes(uint32_t n, int nbits) {
  uint32_t nb = num_tiles(n);
  uint32_t chunk = scan_chunk_rows(nb);
  uint32_t chunks = (nb + chunk - 1) / chunk;
  return (size_t)chunks * (1u << nbits) * sizeof(uint32_t);
}

template <int NBITS>
static void scan_launch(uint32_t* hist, uint32_t nb, uint32_t* partial,
                        uint32_t* totals, hipStream_t s) {
  constexpr int ND = 1 << NBITS;
  uint32_t chunk = scan_chunk_rows(nb);
  uint32_t chunks = (nb + chunk - 1) / chunk;
  hipLaunchKernelGGL(scan_chunk_sums_kernel<ND>, dim3(chunks), dim3(BLOCK), 0,
                     s, hist, nb, chunk, partial);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(scan_chunks_kernel<ND>, dim3(1), dim3(BLOCK), 0, s,
                     partial, chunks, totals);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(scan_rewrite_kernel<ND>, dim3(chunks), dim3(BLOCK), 0, s,
                     hist, nb, chunk, partial);
  HIP_CHECK(hipGetLastError());
}

void radix_scan(uintptr_t hist, uint32_t n, int nbits, uintptr_t totals,
                uintptr_t scan_ws, uintptr_t stream) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  uint32_t nb = num_tiles(n);
  DISPATCH_NBITS(nbits, scan_launch, reinterpret_cast<uint32_t*>(hist), nb,
                 reinterpret_cast<uint32_t*>(scan_ws),
                 reinterpret_cast<uint32_t*>(totals), s);
}

template <int NBITS>
static void scatter_hv(const uint64_t* keys, const uint64_t* vals, uint32_t n,
                       int shift, const uint32_t* hist, const uint64_t* kd,
                       const uint64_t* vd, hipStream_t s, int func = 0,
                       int aos_out = 0, int in_stride = 1,
                       uint32_t nparts = 0) {
  if (vals)
    scatter_launch<NBITS, true>(keys, vals, n, shift, hist, kd, vd, s,
                                func, aos_out, in_stride, nparts);
  else
    scatter_launch<NBITS, false>(keys, nullptr, n, shift, hist, kd, nullptr,
                                 s, func, aos_out, in_stride, nparts);
}

void radix_scatter(uintptr_t keys, uintptr_t vals, uint32_t n, int shift,
                   int nbits, uintptr_t hist, uintptr_t key_dst,
                   uintptr_t val_dst, uintptr_t stream, int func,
                   int aos_out, int in_stride, uint32_t nparts) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_NBITS(nbits, scatter_hv, reinterpret_cast<const uint64_t*>(keys),
                 reinterpret_cast<const uint64_t*>(vals), n, shift,
                 reinterpret_cast<const uint32_t*>(hist),
                 reinterpret_cast<const uint64_t*>(key_dst),
                 reinterpret_cast<const uint64_t*>(val_dst), s, func,
                 aos_out, in_stride, nparts);
}

// Full LSD sort of (keys[, vals]) by bits [start_bit, end_bit).
// ws layout: hist u32[ND*nb] | totals u32[256] | key_dst u64[256] |
//            val_dst u64[256].  Returns which buffer holds the result:
// 0 = keys/vals, 1 = tmp_keys/tmp_vals.
size_t sort_workspace_bytes(uint32_t n) {
  return radix_hist_bytes(n, 8) + radix_scan_ws_bytes(n, 8) + 256 * 4 +
         256 * 8 * 2;
}

// Onesweep sort: ws layout = totals u32[passes*256] | key_dst u64[256] |
// val_dst u64[256] | ticket u32, tie flag u32 (+pad to 16) |
// desc u32[nb*256]. The ticket slot is zeroed before every pass; the tie
// flag is the overflow word of tie_repair_kernel (truncated sort only).
constexpr int OS_ITEMS = 16;  // SoA: 4096-elem tiles @ 256 threads
constexpr int OS_AOS_BS = 512;  // AoS: 4096-elem tiles @ 512 threads,
constexpr int OS_AOS_ITEMS = 8;  // 2 blocks/CU resident
constexpr int OS_TILE = BLOCK * OS_ITEMS;
static_assert(OS_AOS_BS * OS_AOS_ITEMS == OS_TILE, "one tile size");
// optional phase-timing accumulator: u64[4] = {phaseA, exch, lookback, writeout}
static uint64_t* g_timing_buf = nullptr;
void set_timing_buf(uintptr_t p) { g_timing_buf = reinterpret_cast<uint64_t*>(p); }

static inline uint32_t os_num_tiles_t(uint32_t n, int tile) {
  return (uint32_t)(((uint64_t)n + tile - 1) / tile);
}
static inline uint32_t os_num_tiles(uint32_t n) {
  return os_num_tiles_t(n, OS_TILE);
}

size_t onesweep_workspace_bytes(uint32_t n, int passes) {
  // SoA and AoS passes both run OS_TILE-element tiles: the size is exact
  uint32_t nb = os_num_tiles(n);
  return (size_t)passes * 256 * 4 + 256 * 8 * 2 + 16 +
         (size_t)nb * 256 * 8;
}

// The parts of a ws of onesweep_workspace_bytes(n, passes) bytes.
struct OnesweepWs {
  uint32_t* totals;   // [passes][256]
  uint64_t* key_dst;  // [256]
  uint64_t* val_dst;  // [256]
  uint32_t* ticket;   // 4 words: ticket, tie flag, pad
  uint64_t* desc;     // [nb][256]
};
static inline OnesweepWs onesweep_ws(uintptr_t ws, int passes) {
  OnesweepWs w;
  w.totals = reinterpret_cast<uint32_t*>(ws);
  w.key_dst = reinterpret_cast<uint64_t*>(w.totals + (size_t)passes * 256);
  w.val_dst = w.key_dst + 256;
  w.ticket = reinterpret_cast<uint32_t*>(w.val_dst + 256);
  w.desc = reinterpret_cast<uint64_t*>(w.ticket + 4);
  return w;
}

// Dynamic LDS of one pass kernel, and the attribute that lets a launch ask
// for it (more than the 64 KB default), set once on every instantiation
// that is launched: by onesweep_sort and by partition_records_fused.
constexpr size_t OS_LDS_SOA = (size_t)OS_TILE * 8 + (size_t)NW * 256 * 4 +
                              256 * 4 * 2 + BLOCK * 4 + 16 + OS_TILE;
constexpr size_t OS_LDS_AOS = (size_t)OS_TILE * 16 +
                              (size_t)(OS_AOS_BS / kWave) * 256 * 4 +
                              256 * 4 * 2 + OS_AOS_BS * 4 + 16;
static void onesweep_allow_lds() {
  static bool attr_set = false;
  if (attr_set) return;
  for (const void* f :
       {reinterpret_cast<const void*>(
            &onesweep_pass_kernel<true, OS_ITEMS, false, BLOCK>),
        reinterpret_cast<const void*>(
            &onesweep_pass_kernel<false, OS_ITEMS, false, BLOCK>),
        reinterpret_cast<const void*>(
            &onesweep_pass_kernel<true, OS_AOS_ITEMS, true, OS_AOS_BS>),
        reinterpret_cast<const void*>(
            &onesweep_pass_kernel<true, OS_AOS_ITEMS, true, OS_AOS_BS,
                                  true>)})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024 - 1024);
  attr_set = true;
}

// The two buffers a sort ping-pongs between. AoS: keys / tmp_keys point at
// interleaved (key, val) 16-byte pairs and vals / tmp_vals are unused.
// SoA: keys and vals are separate u64 arrays (vals may be 0: keys only).
enum class PairLayout { AoS, SoA };
struct PairBufs {
  uintptr_t keys, tmp_keys;
  uintptr_t vals = 0, tmp_vals = 0;
  PairLayout layout = PairLayout::AoS;
};
// which u64 of an AoS pair a sort orders by: the key prefix, or the aux
// word, whose bits [48, 64) hold the low 16 bits of an 80-bit key
constexpr int kPrefixWord = 0, kAuxWord = 1;
// Where the records of an AoS sort are and where its final pass writes
// them whole, in sorted order. segs / nsegs: record_src (hipshuffle.h).
struct RecordTarget {
  uintptr_t recs, out, segs;
  uint32_t rec_bytes, nsegs;
};
// Tie repair before the final pass of a truncated sort (tie_repair_kernel).
// flag is set by onesweep_sort: the device word of its ws layout, zero
// before the kernel runs, that the kernel raises on a run too long.
struct TieRepair {
  uint64_t run_mask, lo_mask;
  uint32_t* flag = nullptr;
};

// Returns which buffer holds the result: 0 = keys/vals, 1 = the tmp ones;
// -1 when `fuse` was asked for and no pass ran to carry it (an empty bit
// window): nothing is written to fuse->out then. tie needs fuse.
static int onesweep_sort(PairBufs b, uint32_t n, int start_bit, int end_bit,
                         uintptr_t ws, hipStream_t s,
                         int sort_word = kPrefixWord,
                         const RecordTarget* fuse = nullptr,
                         TieRepair* tie = nullptr) {
  constexpr int PBITS = 8;
  constexpr int PD = 1 << PBITS;
  const bool aos = b.layout == PairLayout::AoS;
  // fusion is asked for by naming a record source: recs, or a segment
  // table (record_src), with which recs is unused and may be 0
  const bool want_fuse = fuse && (fuse->recs || fuse->nsegs);
  if (fuse && fuse->nsegs && !fuse->segs)
    throw std::runtime_error("fused sort: nsegs without a table");
  uint32_t nb = os_num_tiles(n);
  int passes = (end_bit - start_bit + PBITS - 1) / PBITS;
  const OnesweepWs w = onesweep_ws(ws, passes);
  uint32_t* totals = w.totals;
  uint64_t *key_dst = w.key_dst, *val_dst = w.val_dst, *desc = w.desc;
  uint32_t* ticket = w.ticket;
  if (tie) tie->flag = ticket + 1;
  HIP_CHECK(hipMemsetAsync(totals, 0, (size_t)passes * PD * 4, s));
  uint32_t hist_grid = nb < 1024 ? (nb ? nb : 1) : 1024;
  hipLaunchKernelGGL((onesweep_hist_all_kernel<10, PBITS>), dim3(hist_grid),
                     dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint64_t*>(b.keys), n, start_bit,
                     passes, totals, aos ? 2 : 1, sort_word);
  HIP_CHECK(hipGetLastError());
  static_assert(PD == 256, "OS_LDS_* are written for 8-bit digits");
  const size_t lds = aos ? OS_LDS_AOS : OS_LDS_SOA;
  onesweep_allow_lds();
  uintptr_t src_k = b.keys, src_v = b.vals, dst_k = b.tmp_keys,
            dst_v = b.tmp_vals;
  int cur = 0;
  for (int p = 0; p < passes; ++p) {
    int sb = start_bit + p * PBITS;
    if (sb > 64 - PBITS) sb = 64 - PBITS;  // same clamp as hist_all
    // fused final pass: the writeout copies whole records to fuse->out
    // (the gather folded into the sort — key_dst becomes record bases)
    const bool fused = want_fuse && aos && p == passes - 1;
    hipLaunchKernelGGL((onesweep_digit_bases_kernel<PD>), dim3(1),
                       dim3(BLOCK), 0, s, totals, p,
                       fused ? (uint64_t)fuse->out : (uint64_t)dst_k,
                       fused ? 0 : (uint64_t)dst_v, key_dst, val_dst,
                       fused ? (int)fuse->rec_bytes : (aos ? 16 : 8));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemsetAsync(ticket, 0, 16, s));
    HIP_CHECK(hipMemsetAsync(desc, 0, (size_t)nb * PD * 8, s));
    if (fused) {
      if (tie) {
        // truncated sort: the passes so far ordered the pairs by the run
        // bits only; put the tied runs in order before the final digit
        hipLaunchKernelGGL(tie_repair_kernel,
                           dim3(os_num_tiles_t(n, TIE_TILE)), dim3(TIE_BS),
                           0, s, reinterpret_cast<uint64_t*>(src_k), n,
                           tie->run_mask, tie->lo_mask, tie->flag);
        HIP_CHECK(hipGetLastError());
      }
      hipLaunchKernelGGL(
          (onesweep_pass_kernel<true, OS_AOS_ITEMS, true, OS_AOS_BS, true>),
          dim3(nb), dim3(OS_AOS_BS), lds, s,
          reinterpret_cast<const uint64_t*>(src_k), nullptr, n, sb, desc,
          ticket, key_dst, val_dst, nullptr, sort_word,
          reinterpret_cast<const uint32_t*>(fuse->recs),
          fuse->rec_bytes / 4,
          reinterpret_cast<const RecSegment*>(fuse->segs), fuse->nsegs);
      HIP_CHECK(hipGetLastError());
      return cur;  // records land in fuse->out; pair buffers are dead
    } else if (aos) {
      hipLaunchKernelGGL(
          (onesweep_pass_kernel<true, OS_AOS_ITEMS, true, OS_AOS_BS>),
          dim3(nb), dim3(OS_AOS_BS), lds, s,
          reinterpret_cast<const uint64_t*>(src_k), nullptr, n, sb, desc,
          ticket, key_dst, val_dst, g_timing_buf, sort_word);
    } else if (b.vals) {
      hipLaunchKernelGGL(
          (onesweep_pass_kernel<true, OS_ITEMS, false, BLOCK>),
          dim3(nb), dim3(BLOCK), lds, s,
          reinterpret_cast<const uint64_t*>(src_k),
          reinterpret_cast<const uint64_t*>(src_v), n, sb, desc, ticket,
          key_dst, val_dst);
    } else {
      hipLaunchKernelGGL(
          (onesweep_pass_kernel<false, OS_ITEMS, false, BLOCK>),
          dim3(nb), dim3(BLOCK), lds, s,
          reinterpret_cast<const uint64_t*>(src_k), nullptr, n, sb, desc,
          ticket, key_dst, val_dst);
    }
    HIP_CHECK(hipGetLastError());
    std::swap(src_k, dst_k);
    std::swap(src_v, dst_v);
    cur ^= 1;
  }
  // a requested fusion with no pass to apply it in (end_bit == start_bit)
  // must NOT silently leave `out` unwritten — the caller falls back
  if (want_fuse) return -1;
  return cur;
}

int onesweep_sort_pairs_u64(uintptr_t keys, uintptr_t vals,
                            uintptr_t tmp_keys, uintptr_t tmp_vals,
                            uint32_t n, int start_bit, int end_bit,
                            uintptr_t ws, uintptr_t stream) {
  return onesweep_sort({keys, tmp_keys, vals, tmp_vals, PairLayout::SoA}, n,
                       start_bit, end_bit, ws,
                       reinterpret_cast<hipStream_t>(stream));
}

// sort_word = 1: the pairs order by their SECOND u64's bits (the aux word
// of the wide-record path).
int onesweep_sort_aos_u64(uintptr_t pairs, uintptr_t tmp_pairs, uint32_t n,
                          int start_bit, int end_bit, uintptr_t ws,
                          uintptr_t stream, int sort_word) {
  return onesweep_sort({pairs, tmp_pairs}, n, start_bit, end_bit, ws,
                       reinterpret_cast<hipStream_t>(stream), sort_word);
}

// ---------------------------------------------------------------------------
// Map-side partition of wide records in one fused pass (digits of at most
// 8 bits). The pairs carry the record's partition id in pair.x, so the
// digit is the id and the fused pass kernel of the sort is the whole job:
// it ranks a tile of pairs, finds the tile's place in every partition by
// look-back and writes the tile's records in per-partition runs, in input
// order. The per-digit record bases are the caller's block addresses, in
// place of the output of onesweep_digit_bases_kernel. The pairs enter in
// input order, so the records a tile reads are one contiguous span of the
// source.

// The 256 totals of pair.x's low byte over n pairs, for the caller's
// layout. No per-tile matrix, no scan.
void count_pair_digits(uintptr_t pairs, uint32_t n, uintptr_t totals,
                       uintptr_t stream) {
  if (pairs % 16 || totals % 4)
    throw std::runtime_error(
        "count_pair_digits: pairs need 16-byte, totals 4-byte alignment");
  auto s = reinterpret_cast<hipStream_t>(stream);
  HIP_CHECK(hipMemsetAsync(reinterpret_cast<void*>(totals), 0, 256 * 4, s));
  if (n == 0) return;
  const uint32_t nb = os_num_tiles(n);
  hipLaunchKernelGGL((onesweep_hist_all_kernel<10, 8>),
                     dim3(nb < 1024 ? nb : 1024), dim3(BLOCK), 0, s,
                     reinterpret_cast<const uint64_t*>(pairs), n,
                     /*start_bit=*/0, /*passes=*/1,
                     reinterpret_cast<uint32_t*>(totals), /*in_stride=*/2,
                     /*word_off=*/0);
  HIP_CHECK(hipGetLastError());
}

size_t partition_records_workspace_bytes(uint32_t n) {
  return onesweep_workspace_bytes(n, 1);
}

// Record idx = pair.y & (2^48 - 1) of `recs` goes to dst_table[pair.x],
// behind the records of the same partition that precede it in the pairs.
// dst_table: device u64[256] of 4-byte-aligned byte addresses; the entry
// of a partition no pair names is never read past the table. pair.x < 256
// and idx < the record count of `recs` are the caller's to guarantee.
// ws: partition_records_workspace_bytes(n), 8-byte aligned.
void partition_records_fused(uintptr_t pairs, uint32_t n, uintptr_t recs,
                             uint32_t rec_bytes, uintptr_t dst_table,
                             uintptr_t ws, uintptr_t stream) {
  if (rec_bytes % 4 || rec_bytes < 4)
    throw std::runtime_error("rec_bytes must be a positive multiple of 4");
  if (pairs % 16 || recs % 4 || dst_table % 8 || ws % 8)
    throw std::runtime_error(
        "partition_records_fused: pairs need 16-byte, recs 4-byte, "
        "dst_table and ws 8-byte alignment");
  if (n == 0) return;
  if (!pairs || !recs || !dst_table || !ws)
    throw std::runtime_error("partition_records_fused: null argument");
  auto s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t nb = os_num_tiles(n);
  const OnesweepWs w = onesweep_ws(ws, 1);
  onesweep_allow_lds();
  HIP_CHECK(hipMemsetAsync(w.ticket, 0, 16, s));
  HIP_CHECK(hipMemsetAsync(w.desc, 0, (size_t)nb * 256 * 8, s));
  hipLaunchKernelGGL(
      (onesweep_pass_kernel<true, OS_AOS_ITEMS, true, OS_AOS_BS, true>),
      dim3(nb), dim3(OS_AOS_BS), OS_LDS_AOS, s,
      reinterpret_cast<const uint64_t*>(pairs), nullptr, n, /*shift=*/0,
      w.desc, w.ticket, reinterpret_cast<const uint64_t*>(dst_table),
      /*val_dst=*/nullptr, /*timing=*/nullptr, /*sort_word=*/kPrefixWord,
      reinterpret_cast<const uint32_t*>(recs), rec_bytes / 4,
      /*rec_segs=*/nullptr, /*rec_nsegs=*/0);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Truncated wide-record sort. After the records are ordered by any
// run_bits consecutive key bits with 2^run_bits >= 8n, a record of a
// non-degenerate input shares those bits with < 1/8 other records on
// average, so LSD passes over the bits below them sort almost nothing.
// Instead: LSD over prefix bits [lo_bit, top) only, tie_repair_kernel on
// the rare tied runs, then the unchanged fused final pass over
// [top, end_bit). Inputs with a run longer than TIE_L fall back to the
// full sequence, so the output never depends on the path taken.

// 0 = always the full LSD sequence; m >= 1 = truncated sort with tie
// repair, using 8 * (m - 1) run bits more than the 8n rule (A/B knob)
static int g_tie_repair = 1;
void set_tie_repair(int m) { g_tie_repair = m < 0 ? 0 : m; }
// path of the latest sort_records_u64 call: 0 = full sequence only,
// 1 = truncated, 2 = truncated then full fallback
static int g_last_sort_path = 0;
int last_sort_path() { return g_last_sort_path; }
int tie_repair_tile() { return TIE_TILE; }
int tie_repair_max_run() { return TIE_L; }

// Digits count DOWN from end_bit so every pass covers 8 live bits: the
// final (fused) digit starts at top = end_bit - 8, the run bits are the
// run_bits below it. passes == 0: the truncated plan does not apply (it
// would leave fewer than 8 low prefix bits, saving under two passes).
void sort_records_plan(uint32_t n, int end_bit, int* lo_bit, int* passes,
                       int* run_bits) {
  if (end_bit > 64) end_bit = 64;
  int rb = 8;
  while (rb < 64 && (1ull << rb) < 8ull * n) rb += 8;
  rb += 8 * (g_tie_repair > 1 ? g_tie_repair - 1 : 0);
  *run_bits = rb;
  *lo_bit = end_bit - 8 - rb;
  *passes = *lo_bit >= 8 ? rb / 8 + 1 : 0;
}

// Passes of the full sequence: the prefix digits of [0, end_bit) and, for
// keys longer than the prefix, the two of the aux word.
static int record_sort_passes(int end_bit, int key_bytes) {
  end_bit = end_bit < 0 ? 0 : end_bit > 64 ? 64 : end_bit;
  return (end_bit + 7) / 8 + (key_bytes > 8 ? 2 : 0);
}

// ws of sort_records_u64: the onesweep layout of the full sequence. The
// tie-repair overflow flag has its word in every onesweep layout (the
// ticket slot), so the truncated plan's own layout holds it.
size_t sort_records_workspace_bytes(uint32_t n, int end_bit, int key_bytes) {
  return onesweep_workspace_bytes(n, record_sort_passes(end_bit, key_bytes));
}

// The full LSD sequence over the 80-bit key, on the pairs as they stand in
// b.keys: 16 aux bits first when the key has them, then the prefix bits
// [0, end_bit). With `fuse` the final prefix pass writes the records to
// t.out itself; without it, or with no pass to carry it (end_bit == 0),
// the pairs are sorted plainly and gather_records moves the records.
static void sort_records_full(PairBufs b, uint32_t n, int end_bit,
                              int key_bytes, uintptr_t ws, hipStream_t s,
                              const RecordTarget& t, bool fuse) {
  if (key_bytes > 8 && onesweep_sort(b, n, 48, 64, ws, s, kAuxWord))
    std::swap(b.keys, b.tmp_keys);
  if (fuse && onesweep_sort(b, n, 0, end_bit, ws, s, kPrefixWord, &t) >= 0)
    return;
  if (onesweep_sort(b, n, 0, end_bit, ws, s)) std::swap(b.keys, b.tmp_keys);
  gather_records(t.recs, b.keys, n, t.rec_bytes, /*dst_mode=*/0, t.out,
                 /*dst_addr=*/0, /*dstart=*/0, /*shift=*/0, /*mask=*/0,
                 /*func=*/0, /*nparts=*/0, reinterpret_cast<uintptr_t>(s),
                 t.segs, t.nsegs);
}

// Sorts the extracted pairs and writes the sorted RECORDS to `out`, by the
// truncated sort when `fuse` and tie repair are on and sort_records_plan
// has a plan, else by the full sequence. Returns the path taken, which
// last_sort_path() repeats. ws: sort_records_workspace_bytes.
// BLOCKS on the stream once, and only after a truncated attempt (the flag
// decides whether to fall back).
int sort_records_u64(uintptr_t pairs, uintptr_t tmp_pairs, uint32_t n,
                     int end_bit, int key_bytes, uintptr_t ws,
                     uintptr_t stream, uintptr_t recs, uintptr_t out,
                     uint32_t rec_bytes, int fuse, uintptr_t segs,
                     uint32_t nsegs) {
  g_last_sort_path = 0;
  if (n == 0) return 0;
  end_bit = end_bit < 0 ? 0 : end_bit > 64 ? 64 : end_bit;
  auto s = reinterpret_cast<hipStream_t>(stream);
  PairBufs b{pairs, tmp_pairs};
  const RecordTarget target{recs, out, segs, rec_bytes, nsegs};
  int lo_bit, passes = 0, run_bits;
  if (fuse && g_tie_repair)
    sort_records_plan(n, end_bit, &lo_bit, &passes, &run_bits);
  if (passes == 0) {
    sort_records_full(b, n, end_bit, key_bytes, ws, s, target, fuse);
    return 0;
  }
  // ws is sized for the full sequence; a plan leaves the low bits out
  // (lo_bit >= 8: passes < ceil(end_bit / 8)), so its layout is shorter
  const int top = end_bit - 8;
  const uint64_t lo_mask = (1ull << lo_bit) - 1;
  TieRepair tie{((1ull << top) - 1) & ~lo_mask, lo_mask};
  int cur = onesweep_sort(b, n, lo_bit, end_bit, ws, s, kPrefixWord, &target,
                          &tie);
  // the plan covers >= 2 digits, so the fused pass ran
  if (cur < 0) throw std::runtime_error("truncated sort: no pass ran");
  uint32_t overflow = 0;
  HIP_CHECK(hipMemcpyAsync(&overflow, tie.flag, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (!overflow) return g_last_sort_path = 1;
  // some run was too long to repair: the full sequence on the pairs as
  // they now stand. Every step so far was stable, so equal full keys are
  // still in input order and the LSD sort gives the same output; `out` is
  // simply overwritten.
  if (cur == 1) std::swap(b.keys, b.tmp_keys);
  sort_records_full(b, n, end_bit, key_bytes, ws, s, target, fuse);
  return g_last_sort_path = 2;
}

int sort_pairs_u64(uintptr_t keys, uintptr_t vals, uintptr_t tmp_keys,
                   uintptr_t tmp_vals, uint32_t n, int start_bit, int end_bit,
                   uintptr_t ws, uintptr_t stream) {
  auto s = reinterpret_cast<hipStream_t>(stream);
  uint32_t nb = num_tiles(n);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
  uint32_t* scan_ws = hist + (size_t)256 * nb;
  uint32_t* totals = scan_ws + radix_scan_ws_bytes(n, 8) / 4;
  uint64_t* key_dst = reinterpret_cast<uint64_t*>(totals + 256);
  uint64_t* val_dst = key_dst + 256;
  uintptr_t src_k = keys, src_v = vals, dst_k = tmp_keys, dst_v = tmp_vals;
  int cur = 0;
  for (int bit = start_bit; bit < end_bit; bit += 8) {
    hist_launch<8>(reinterpret_cast<const uint64_t*>(src_k), n, bit, hist, s);
    scan_launch<8>(hist, nb, scan_ws, totals, s);
    hipLaunchKernelGGL(radix_digit_bases_kernel<8>, dim3(1), dim3(BLOCK), 0, s,
                       totals, (uint64_t)dst_k, (uint64_t)dst_v, key_dst,
                       val_dst);
    HIP_CHECK(hipGetLastError());
    scatter_hv<8>(reinterpret_cast<const uint64_t*>(src_k),
                  reinterpret_cast<const uint64_t*>(src_v), n, bit, hist,
                  key_dst, val_dst, s);
    std::swap(src_k, dst_k);
    std::swap(src_v, dst_v);
    cur ^= 1;
  }
  return cur;
}

}  // namespace hipshuffle
