// Sort-merge join family over key-sorted SoA (u64 key, u64 payload) tables
// for MI355X (gfx950): inner, left / right / full outer, left semi and left
// anti — the join types of Spark's SortMergeJoinExec, which the reference
// plugin's reducers serve. The inner-only pair join_count / join_emit of
// kernels.hip stays as it is; this file is a separate translation unit.
//
// P is the probing (driving) side, Q the side that is searched; both are
// sorted by key, compared as UNSIGNED 64-bit over all 64 bits.
//
// Scheme — two kernels, the scan between them is plumbing (ops/join.py):
//
//   probe    one thread per P row i:
//              lo[i] = lower_bound(Q, pkey[i])      binary search
//              m[i]  = upper_bound(Q, pkey[i]) - lo[i]
//            The upper bound gallops from lo (probe lo+1, lo+2, lo+4, ...)
//            and finishes with a binary search inside the last bracket:
//            O(log run) <= O(log nq) loads, no linear walk. A row with no
//            match costs one load after the lower bound.
//            A block's 256 P rows are sorted, so its first and last key
//            bound the window of Q it can touch. Two waves find the
//            window's ends (wave_count_below: 64-ary narrowing with a
//            ballot, 4 dependent loads for 2^24 rows); a window of at most
//            PROBE_LDS_KEYS keys is staged in LDS with coalesced loads and
//            every row searches LDS, a longer one is searched in place.
//            Measured against searching all of Q from global memory per
//            row: 0.22 vs 0.38 ms per 2^24 x 2^24 rows
//            (profiles/r11_join_family.md).
//   count    c[i] from m[i] by join type: inner m, left outer max(m, 1),
//            semi m > 0, anti m == 0; offsets = exclusive scan (int64)
//   expand   OUTPUT-centric: a block owns EXPAND_TILE consecutive output
//            rows. Two waves find the first and the last owning P row with
//            one wave_count_below each over offsets[]. Every thread resolves
//            its output row o to the owner i = upper_bound(offsets, o) - 1
//            (the LAST row with offsets[i] <= o: rows with c == 0 share an
//            offset with their successor and are never chosen) and to
//            j = o - offsets[i], then writes the requested SoA outputs.
//            Consecutive lanes write consecutive rows of every output and
//            read consecutive Q rows inside a run; per-thread work is the
//            search, never a run length.
//
//   The owner search runs over the block's range [i0, i1] only. When the
//   range has at most EXPAND_LDS_ROWS rows it is staged in LDS as u32
//   offsets relative to the tile's first row (every offset but the first
//   lies inside the tile; the first is clamped to 0 for the search and its
//   true value kept in a register for j). A longer range — a tile that
//   spans a long stretch of rows with c == 0 — is searched in global
//   memory (L2-resident: the block's probes share the top of the tree).
//
// Semi and anti are the same expand with c in {0, 1} and no Q outputs: a
// stream compaction. Full outer is two expands (ops/join.py): left outer
// of A into out[0:T1], then anti of B probing A into out[T1:T1+T2].
//
// No atomics, no block waits on another block, plain vector stores only.
// Limits: np, nq < 2^31; offsets and totals are 64-bit.

#include "common.h"
#include "hipshuffle.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int JOIN_BLOCK = 256;
constexpr int EXPAND_ITEMS = 8;
constexpr int EXPAND_TILE = JOIN_BLOCK * EXPAND_ITEMS;      // output rows
constexpr uint32_t EXPAND_LDS_ROWS = 2 * EXPAND_TILE;       // 16 KB of u32
constexpr uint32_t JOIN_MAX_ROWS = 0x7fffffffu;

constexpr uint32_t PROBE_LDS_KEYS = 2048;                   // 16 KB of u64

// lower bound of key in arr[0, n), then the length of its run: gallop from
// the lower bound (probe +1, +2, +4, ...), then bisect the last bracket
template <typename Ptr>
__device__ __forceinline__ void probe_row(Ptr arr, uint32_t n, uint64_t k,
                                          uint32_t* lo_out, uint32_t* m_out) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (arr[mid] < k) lo = mid + 1; else hi = mid;
  }
  uint32_t m = 0;
  if (lo < n && arr[lo] == k) {
    // invariant: arr[lo + a] == k, and b is n - lo or arr[lo + b] > k
    uint32_t a = 0, b = n - lo, step = 1;
    while (a + step < b) {
      if (arr[lo + a + step] == k) {
        a += step;
        step <<= 1;
      } else {
        b = a + step;
      }
    }
    while (b - a > 1) {                // the run ends inside (a, b]
      const uint32_t mid = a + ((b - a) >> 1);
      if (arr[lo + mid] == k) a = mid; else b = mid;
    }
    m = a + 1;
  }
  *lo_out = lo;
  *m_out = m;
}

// Every Q row equal to a key of the block lies in the window
// [#{Q < first key}, #{Q <= last key}), and so does every lower bound.
__global__ __launch_bounds__(JOIN_BLOCK) void join_probe_kernel(
    const uint64_t* __restrict__ pkey, uint32_t np,
    const uint64_t* __restrict__ qkey, uint32_t nq,
    uint32_t* __restrict__ lo_out, uint32_t* __restrict__ m_out) {
  __shared__ uint64_t s_q[PROBE_LDS_KEYS];
  __shared__ uint32_t s_win[2];
  const uint32_t t = threadIdx.x;
  const uint32_t base = blockIdx.x * JOIN_BLOCK;     // < np: grid = ceil
  const uint32_t i = base + t;
  const uint32_t rows = min((uint32_t)JOIN_BLOCK, np - base);
  const uint32_t wv = t / kWave, lane = t & (kWave - 1);
  if (wv == 0) {
    const uint32_t w = wave_count_below<true>(qkey, nq, pkey[base], lane);
    if (lane == 0) s_win[0] = w;
  } else if (wv == 1) {
    const uint32_t w =
        wave_count_below<false>(qkey, nq, pkey[base + rows - 1], lane);
    if (lane == 0) s_win[1] = w;
  }
  __syncthreads();
  const uint32_t w0 = s_win[0], wn = s_win[1] - w0;   // block-uniform
  uint32_t lo = 0, m = 0;
  if (wn <= PROBE_LDS_KEYS) {
    for (uint32_t r = t; r < wn; r += JOIN_BLOCK) s_q[r] = qkey[w0 + r];
    __syncthreads();
    if (i < np) probe_row(s_q, wn, pkey[i], &lo, &m);
  } else if (i < np) {
    probe_row(qkey + w0, wn, pkey[i], &lo, &m);
  }
  if (i < np) {
    lo_out[i] = w0 + lo;
    m_out[i] = m;
  }
}

struct ExpandArgs {
  const uint64_t* pkey;
  const uint64_t* pval;
  const uint64_t* qval;
  const uint32_t* lo;
  const uint32_t* m;
  const uint64_t* offsets;
  uint32_t np;
  uint64_t total;
  uint64_t* out_key;
  uint64_t* out_p_val;
  uint64_t* out_q_val;
  uint8_t* out_q_valid;
  int64_t* out_p_idx;
  int64_t* out_q_idx;
};

// output row o is match j of P row i
__device__ __forceinline__ void join_emit_row(const ExpandArgs& p, uint64_t o,
                                              uint32_t i, uint64_t j) {
  if (p.out_key) p.out_key[o] = p.pkey[i];
  if (p.out_p_val) p.out_p_val[o] = p.pval[i];
  if (p.out_p_idx) p.out_p_idx[o] = (int64_t)i;
  if (p.out_q_val || p.out_q_valid || p.out_q_idx) {
    const bool hit = p.m[i] != 0;
    const uint64_t q = hit ? (uint64_t)p.lo[i] + j : 0;
    if (p.out_q_val) p.out_q_val[o] = hit ? p.qval[q] : 0;
    if (p.out_q_valid) p.out_q_valid[o] = hit ? 1 : 0;
    if (p.out_q_idx) p.out_q_idx[o] = hit ? (int64_t)q : -1;
  }
}

__global__ __launch_bounds__(JOIN_BLOCK) void join_expand_kernel(
    const ExpandArgs p) {
  __shared__ uint32_t s_rel[EXPAND_LDS_ROWS];
  __shared__ uint32_t s_rng[2];
  const uint32_t t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * EXPAND_TILE;
  const uint64_t rem = p.total - tile0;          // > 0: grid = ceil(total/T)
  const uint32_t rows = rem < EXPAND_TILE ? (uint32_t)rem : EXPAND_TILE;

  // owners of the tile's first and last row; offsets[0] == 0 <= any row,
  // so the count of offsets <= o is at least 1
  if (t < 2 * kWave) {                           // waves 0 and 1, whole
    const uint32_t wv = t / kWave, lane = t & (kWave - 1);
    const uint64_t o = wv ? tile0 + rows - 1 : tile0;
    const uint32_t c = wave_count_below<false>(p.offsets, p.np, o, lane);
    if (lane == 0) s_rng[wv] = c - 1;
  }
  __syncthreads();
  const uint32_t i0 = s_rng[0];
  const uint32_t cnt = s_rng[1] - i0 + 1;        // block-uniform

  if (cnt <= EXPAND_LDS_ROWS) {
    // offsets[i0] <= tile0 < offsets[i0 + r] < tile0 + rows for r >= 1
    const uint64_t off0 = p.offsets[i0];
    for (uint32_t r = t; r < cnt; r += JOIN_BLOCK)
      s_rel[r] = r ? (uint32_t)(p.offsets[i0 + r] - tile0) : 0;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < EXPAND_ITEMS; ++it) {
      const uint32_t x = it * JOIN_BLOCK + t;    // row inside the tile
      if (x < rows) {
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_rel[mid] <= x) lo = mid + 1; else hi = mid;
        }
        const uint32_t r = lo - 1;
        const uint64_t j = r ? (uint64_t)(x - s_rel[r]) : tile0 + x - off0;
        join_emit_row(p, tile0 + x, i0 + r, j);
      }
    }
  } else {
    const uint64_t* __restrict__ off = p.offsets + i0;
#pragma unroll 1
    for (int it = 0; it < EXPAND_ITEMS; ++it) {
      const uint32_t x = it * JOIN_BLOCK + t;
      if (x < rows) {
        const uint64_t o = tile0 + x;
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (off[mid] <= o) lo = mid + 1; else hi = mid;
        }
        const uint32_t r = lo - 1;
        join_emit_row(p, o, i0 + r, o - off[r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers

int join_expand_tile() { return EXPAND_TILE; }
int join_expand_lds_rows() { return (int)EXPAND_LDS_ROWS; }
int join_probe_lds_keys() { return (int)PROBE_LDS_KEYS; }

void join_probe(uintptr_t p_keys, uint32_t np, uintptr_t q_keys, uint32_t nq,
                uintptr_t lo, uintptr_t m, uintptr_t stream) {
  if (np == 0) return;
  if (np > JOIN_MAX_ROWS || nq > JOIN_MAX_ROWS)
    throw std::invalid_argument("join_probe: row count exceeds 2^31 - 1");
  if (!p_keys || !lo || !m || (nq && !q_keys))
    throw std::invalid_argument("join_probe: null buffer");
  if ((p_keys & 7) || (q_keys & 7) || (lo & 3) || (m & 3))
    throw std::invalid_argument("join_probe: misaligned buffer");
  const uint32_t grid = (np + JOIN_BLOCK - 1) / JOIN_BLOCK;
  hipLaunchKernelGGL(join_probe_kernel, dim3(grid), dim3(JOIN_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint64_t*>(p_keys), np,
                     reinterpret_cast<const uint64_t*>(q_keys), nq,
                     reinterpret_cast<uint32_t*>(lo),
                     reinterpret_cast<uint32_t*>(m));
  HIP_CHECK(hipGetLastError());
}

void join_expand(uintptr_t p_keys, uintptr_t p_vals, uintptr_t q_vals,
                 uintptr_t lo, uintptr_t m, uintptr_t offsets, uint32_t np,
                 uint64_t total, uintptr_t out_key, uintptr_t out_p_val,
                 uintptr_t out_q_val, uintptr_t out_q_valid,
                 uintptr_t out_p_idx, uintptr_t out_q_idx,
                 uintptr_t stream) {
  if (total == 0) return;
  if (np == 0 || np > JOIN_MAX_ROWS)
    throw std::invalid_argument("join_expand: np must be in [1, 2^31 - 1]");
  const uint64_t grid = (total + EXPAND_TILE - 1) / EXPAND_TILE;
  if (grid > 0x7fffffffull)
    throw std::invalid_argument("join_expand: total exceeds the grid limit");
  if (!offsets) throw std::invalid_argument("join_expand: offsets is null");
  if (out_key && !p_keys)
    throw std::invalid_argument("join_expand: out_key without p_keys");
  if (out_p_val && !p_vals)
    throw std::invalid_argument("join_expand: out_p_val without p_vals");
  if ((out_q_val || out_q_valid || out_q_idx) && (!lo || !m))
    throw std::invalid_argument("join_expand: Q outputs need lo and m");
  if (out_q_val && !q_vals)
    throw std::invalid_argument("join_expand: out_q_val without q_vals");
  if (((p_keys | p_vals | q_vals | offsets | out_key | out_p_val |
        out_q_val | out_p_idx | out_q_idx) & 7) || ((lo | m) & 3))
    throw std::invalid_argument("join_expand: misaligned buffer");
  ExpandArgs a;
  a.pkey = reinterpret_cast<const uint64_t*>(p_keys);
  a.pval = reinterpret_cast<const uint64_t*>(p_vals);
  a.qval = reinterpret_cast<const uint64_t*>(q_vals);
  a.lo = reinterpret_cast<const uint32_t*>(lo);
  a.m = reinterpret_cast<const uint32_t*>(m);
  a.offsets = reinterpret_cast<const uint64_t*>(offsets);
  a.np = np;
  a.total = total;
  a.out_key = reinterpret_cast<uint64_t*>(out_key);
  a.out_p_val = reinterpret_cast<uint64_t*>(out_p_val);
  a.out_q_val = reinterpret_cast<uint64_t*>(out_q_val);
  a.out_q_valid = reinterpret_cast<uint8_t*>(out_q_valid);
  a.out_p_idx = reinterpret_cast<int64_t*>(out_p_idx);
  a.out_q_idx = reinterpret_cast<int64_t*>(out_q_idx);
  hipLaunchKernelGGL(join_expand_kernel, dim3((uint32_t)grid),
                     dim3(JOIN_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace hipshuffle
