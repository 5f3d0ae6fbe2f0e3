// Segmented reduce of up to 8 typed columns of W-byte records, over
// key-sorted 16-byte (u64 key, u64 aux) pairs, for MI355X (gfx950) — the
// GROUP BY of the wide-record lane. The records are never moved: the pair
// machinery (extract_pairs, sort_pairs_aos) leaves (key, record index)
// pairs, and this kernel reads each record's few column bytes where the
// record lies — contiguous, or through the segment table of record_src,
// i.e. inside the shuffle's own blocks for an in-place reader.
//
// Heads, runs and the output order are reduce.hip's: element i is a HEAD
// iff i == 0 or key[i] != key[i-1] (all 64 bits); output is SoA, out_keys
// u64[g] and column c at out_vals + c * g, one row per run in input order.
//
// A column is {word offset, type, op}. Integers widen to i64 (i32 sign-,
// u32 zero-extended), floats to f64; `sum` wraps mod 2^64 or adds f64 in a
// fixed order, `min` / `max` compare signed i64 or IEEE f64, `count` is the
// run length and reads nothing. Records are only 4-byte aligned, so an
// 8-byte field is two dword loads; no byte outside [0, rec_bytes) is read.
//
// Scheme — reduce.hip's: ONE kernel template launched twice, the scan of
// per-tile head counts between the launches (plumbing in ops/radix.py).
//
//   tile = 256 threads x 8 records. Keys and one column's values at a time
//   go lane-linear into padded LDS and come back thread-linear (a thread
//   owns 8 consecutive records).
//
//   count launch  reads the pairs coalesced, keeps the 8 record addresses
//                 of a lane in registers and, per column, issues the loads
//                 of all 8 records (8 or 16 dwords in flight per lane)
//                 before the first use; widens; writes the values to a
//                 dense u64 [C][n] scratch in sorted order (coalesced) and
//                 to LDS. heads[b] = heads in tile b; lead[c][b] = column
//                 c's reduction of the records before tile b's first head.
//   scan          base[b] = exclusive sum of heads
//   emit launch   streams the scratch — it never touches a record — runs
//                 the same in-tile segmented reduction per column, and wave
//                 0 walks forward over lead[c][b+1], ... for the run that
//                 is open at the tile's end.
//
// Each record is therefore read from its source once per call. No atomics,
// no block waits on a concurrently running block, and every combine order
// is fixed by (n, tile geometry) alone: f64 sums are bit-reproducible, and
// independent of where the records lie.
//
// The op is a run-time, grid-uniform value (the column table is a kernel
// argument): one uniform switch per column picks the in-tile reduction
// compiled for its accumulator kind. That reduction is copied from
// reduce.hip rather than shared, which leaves reduce_by_key_kernel's code
// and resource usage exactly as they were.

#include "common.h"
#include "hipshuffle.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int RR_BLOCK = 256;
constexpr int RR_ITEMS = 8;
constexpr int RR_TILE = RR_BLOCK * RR_ITEMS;
constexpr int RR_WAVES = RR_BLOCK / kWave;
constexpr int RR_MAX_COLS = 8;

enum { RR_I32 = 0, RR_U32 = 1, RR_I64 = 2, RR_F32 = 3, RR_F64 = 4 };
enum { RR_SUM = 0, RR_MIN = 1, RR_MAX = 2, RR_COUNT = 3 };
// accumulator kinds: what (type, op) folds with
enum { RR_ADD_I = 0, RR_ADD_F = 1, RR_MIN_I = 2, RR_MAX_I = 3, RR_MIN_F = 4,
       RR_MAX_F = 5 };

struct RrColumn {
  uint16_t off;  // first word of the field inside the record
  uint8_t type;
  uint8_t op;
};

struct RrColumns {
  RrColumn c[RR_MAX_COLS];
};

__device__ __forceinline__ int rr_kind(RrColumn col) {
  const bool f = col.type >= RR_F32;
  switch (col.op) {
    case RR_SUM: return f ? RR_ADD_F : RR_ADD_I;
    case RR_MIN: return f ? RR_MIN_F : RR_MIN_I;
    case RR_MAX: return f ? RR_MAX_F : RR_MAX_I;
    default: return RR_ADD_I;  // count
  }
}

__device__ __forceinline__ uint64_t rr_identity(int kind) {
  switch (kind) {
    case RR_ADD_F: return 0x8000000000000000ull;  // -0.0, see reduce.hip
    case RR_MIN_I: return 0x7fffffffffffffffull;
    case RR_MAX_I: return 0x8000000000000000ull;
    case RR_MIN_F: return 0x7ff0000000000000ull;  // +inf
    case RR_MAX_F: return 0xfff0000000000000ull;  // -inf
    default: return 0;
  }
}

template <int KIND>
__device__ __forceinline__ uint64_t rr_op(uint64_t a, uint64_t b) {
  if constexpr (KIND == RR_ADD_F) {
    return (uint64_t)__double_as_longlong(
        __longlong_as_double((long long)a) + __longlong_as_double((long long)b));
  } else if constexpr (KIND == RR_MIN_I) {
    return (int64_t)a < (int64_t)b ? a : b;
  } else if constexpr (KIND == RR_MAX_I) {
    return (int64_t)a > (int64_t)b ? a : b;
  } else if constexpr (KIND == RR_MIN_F) {
    return __longlong_as_double((long long)b) <
                   __longlong_as_double((long long)a) ? b : a;
  } else if constexpr (KIND == RR_MAX_F) {
    return __longlong_as_double((long long)b) >
                   __longlong_as_double((long long)a) ? b : a;
  } else {
    return a + b;
  }
}

// the accumulator bits of a field read as (lo, hi) dwords
__device__ __forceinline__ uint64_t rr_widen(int type, uint32_t lo,
                                             uint32_t hi) {
  switch (type) {
    case RR_I32: return (uint64_t)(int64_t)(int32_t)lo;
    case RR_U32: return (uint64_t)lo;
    case RR_F32:
      return (uint64_t)__double_as_longlong((double)__uint_as_float(lo));
    default: return ((uint64_t)hi << 32) | lo;
  }
}

__device__ __forceinline__ uint64_t rr_shfl_up(uint64_t v, int d) {
  return (uint64_t)__shfl_up((unsigned long long)v, d, kWave);
}

// record r of the tile sits in slot r + r/8: a thread's 8 records start at
// slot 9t, a 72-byte stride that spreads the 8-byte reads over the banks
__device__ __forceinline__ uint32_t rr_slot(uint32_t r) { return r + (r >> 3); }

// The in-tile segmented reduction of one column (reduce.hip's, copied), on
// the thread-linear values v[] of a thread's m records. EMIT == false leaves
// clead[b]; EMIT == true writes the column's runs to ov[] and walks forward
// over clead[b + 1], ... for the run open at the tile's end. Ends in no
// barrier: the caller synchronises before w_val / w_flag are written again.
template <int KIND, bool EMIT>
__device__ __forceinline__ void rr_reduce_tile(
    const uint64_t (&v)[RR_ITEMS], int m, uint32_t hmask, uint32_t hc,
    uint32_t excl, uint32_t H, uint64_t rank0, uint64_t ident,
    uint64_t* w_val, uint32_t* w_flag, const uint32_t* heads,
    uint64_t* clead, const uint64_t* __restrict__ base, uint64_t* ov) {
  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const uint32_t b = blockIdx.x, nb = gridDim.x;

  // thread-serial: prefix = records before the first head, acc ends as
  // the open suffix (or the thread's total when it holds no head); runs
  // that open and close inside the thread are written here
  uint64_t acc = ident, prefix = ident;
  uint32_t seen = 0;
#pragma unroll
  for (int j = 0; j < RR_ITEMS; ++j) {
    if (j < m) {
      if ((hmask >> j) & 1) {
        if (seen == 0) {
          prefix = acc;
        } else if (EMIT) {
          ov[rank0 + seen - 1] = acc;
        }
        acc = v[j];
        ++seen;
      } else {
        acc = rr_op<KIND>(acc, v[j]);
      }
    }
  }

  // wave64 segmented inclusive scan: a thread with a head starts a segment
  uint64_t sv = acc;
  uint32_t sf = hc > 0;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t uv = rr_shfl_up(sv, d);
    const uint32_t uf = __shfl_up(sf, d, kWave);
    if (lane >= (uint32_t)d) {
      if (!sf) sv = rr_op<KIND>(uv, sv);
      sf |= uf;
    }
  }
  uint64_t xv = rr_shfl_up(sv, 1);
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
  for (int w = 0; w < RR_WAVES; ++w) {
    const uint64_t wvv = w_val[w];
    tail = w_flag[w] ? wvv : rr_op<KIND>(tail, wvv);
    if ((uint32_t)w + 1 == wv) cv = tail;
  }
  const uint64_t carry = xf ? xv : rr_op<KIND>(cv, xv);

  if (hc > 0) {
    // closes the run that was open at this thread's first head
    const uint64_t closed = rr_op<KIND>(carry, prefix);
    if (excl > 0) {
      if (EMIT) ov[rank0 - 1] = closed;
    } else if (!EMIT) {
      clead[b] = closed;  // began before this tile
    }
  }
  if constexpr (!EMIT) {
    if (t == 0 && H == 0) clead[b] = tail;
  } else {
    // forward walk by wave 0: the tile's last run, open at the tile's end
    if (wv == 0 && H > 0) {
      uint64_t run = tail;
      for (uint64_t s0 = (uint64_t)b + 1; s0 < nb; s0 += kWave) {
        const uint64_t tb = s0 + lane;
        const bool in = tb < nb;
        const uint32_t h = in ? heads[tb] : 0;
        uint64_t l = in ? clead[tb] : ident;
        const unsigned long long bal = __ballot(in && h > 0);
        const uint32_t first =
            bal ? (uint32_t)__ffsll((long long)bal) - 1 : kWave;
        if (lane > first) l = ident;
#pragma unroll
        for (int d = kWave / 2; d >= 1; d >>= 1) {
          const uint64_t o =
              (uint64_t)__shfl_down((unsigned long long)l, d, kWave);
          l = rr_op<KIND>(l, o);
        }
        run = rr_op<KIND>(run,
                    (uint64_t)__shfl((unsigned long long)l, 0, kWave));
        if (bal) break;
      }
      if (lane == 0) ov[base[b] + H - 1] = run;
    }
  }
}

// EMIT == false: the count launch (reads the records; writes scratch,
// heads[b], lead[c][b]). EMIT == true: the emit launch (reads scratch,
// heads, lead, base; writes out_*).
template <bool EMIT>
__global__ __launch_bounds__(RR_BLOCK) void reduce_records_kernel(
    const ulonglong2* __restrict__ pairs, uint32_t n,
    const uint32_t* __restrict__ recs, const RecSegment* __restrict__ segs,
    uint32_t nsegs, uint32_t w4, RrColumns cols, uint32_t ncols,
    uint64_t* scratch, uint32_t* heads, uint64_t* lead,
    const uint64_t* __restrict__ base, uint64_t g,
    uint64_t* __restrict__ out_keys, uint64_t* __restrict__ out_vals) {
  __shared__ uint64_t stage_k[RR_TILE + RR_TILE / 8];
  __shared__ uint64_t stage_v[RR_TILE + RR_TILE / 8];
  __shared__ uint64_t w_val[RR_WAVES];
  __shared__ uint32_t w_flag[RR_WAVES];
  __shared__ uint32_t w_heads[RR_WAVES];

  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const uint32_t b = blockIdx.x, nb = gridDim.x;
  const uint64_t tile0 = (uint64_t)b * RR_TILE;

  // lane-linear: keys to LDS; the count launch keeps the record addresses
  const uint32_t* src[RR_ITEMS];
#pragma unroll
  for (int j = 0; j < RR_ITEMS; ++j) {
    const uint32_t r = j * RR_BLOCK + t;
    src[j] = nullptr;
    if (tile0 + r < n) {
      if constexpr (EMIT) {
        stage_k[rr_slot(r)] = pairs[tile0 + r].x;
      } else {
        const ulonglong2 p = pairs[tile0 + r];
        stage_k[rr_slot(r)] = p.x;
        src[j] = record_src(recs, segs, nsegs, p.y & AUX_IDX_MASK, w4);
      }
    }
  }
  __syncthreads();

  const uint64_t i0 = tile0 + (uint64_t)t * RR_ITEMS;
  const int m = i0 >= n ? 0 : (n - i0 < RR_ITEMS ? (int)(n - i0) : RR_ITEMS);
  uint64_t k[RR_ITEMS];
#pragma unroll
  for (int j = 0; j < RR_ITEMS; ++j) k[j] = j < m ? stage_k[9 * t + j] : 0;
  uint64_t prev = 0;
  if (m > 0 && i0 > 0) prev = t ? stage_k[9 * t - 2] : pairs[tile0 - 1].x;

  // head flags and this thread's head count
  uint32_t hmask = 0;
#pragma unroll
  for (int j = 0; j < RR_ITEMS; ++j) {
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
  for (int w = 0; w < RR_WAVES; ++w) {
    if ((uint32_t)w < wv) excl += w_heads[w];
    H += w_heads[w];
  }
  const uint64_t rank0 = EMIT ? base[b] + excl : 0;

  if constexpr (EMIT) {
    uint32_t seen = 0;
#pragma unroll
    for (int j = 0; j < RR_ITEMS; ++j) {
      if (j < m && ((hmask >> j) & 1)) out_keys[rank0 + seen++] = k[j];
    }
  } else {
    if (t == 0) heads[b] = H;
  }

  for (uint32_t c = 0; c < ncols; ++c) {
    const RrColumn col = cols.c[c];
    const int kind = rr_kind(col);
    const uint64_t ident = rr_identity(kind);
    const bool counting = col.op == RR_COUNT;
    uint64_t* colscratch = scratch + (uint64_t)c * n;
    uint64_t* ov = EMIT ? out_vals + (uint64_t)c * g : nullptr;

    __syncthreads();  // the previous column is done with stage_v and w_*
    if (!counting) {
      if constexpr (EMIT) {
#pragma unroll
        for (int j = 0; j < RR_ITEMS; ++j) {
          const uint32_t r = j * RR_BLOCK + t;
          if (tile0 + r < n) stage_v[rr_slot(r)] = colscratch[tile0 + r];
        }
      } else {
        // every load of the lane's 8 records is issued before the first
        // widened value is used
        uint32_t lo[RR_ITEMS], hi[RR_ITEMS];
        const bool wide = col.type == RR_I64 || col.type == RR_F64;
#pragma unroll
        for (int j = 0; j < RR_ITEMS; ++j) {
          lo[j] = src[j] ? src[j][col.off] : 0;
          hi[j] = 0;
        }
        if (wide) {
#pragma unroll
          for (int j = 0; j < RR_ITEMS; ++j)
            hi[j] = src[j] ? src[j][col.off + 1] : 0;
        }
#pragma unroll
        for (int j = 0; j < RR_ITEMS; ++j) {
          const uint32_t r = j * RR_BLOCK + t;
          if (tile0 + r < n) {
            const uint64_t v = rr_widen(col.type, lo[j], hi[j]);
            colscratch[tile0 + r] = v;
            stage_v[rr_slot(r)] = v;
          }
        }
      }
    }
    __syncthreads();

    uint64_t v[RR_ITEMS];
#pragma unroll
    for (int j = 0; j < RR_ITEMS; ++j)
      v[j] = j < m ? (counting ? 1 : stage_v[9 * t + j]) : ident;

    // one uniform switch per column; the reduction itself is compiled per
    // accumulator kind, as reduce.hip's is per op
#define RR_KIND(K)                                                          \
  case K:                                                                   \
    rr_reduce_tile<K, EMIT>(v, m, hmask, hc, excl, H, rank0, ident, w_val,  \
                            w_flag, heads, lead + (uint64_t)c * nb, base,   \
                            ov);                                            \
    break;
    switch (kind) {
      RR_KIND(RR_ADD_I)
      RR_KIND(RR_ADD_F)
      RR_KIND(RR_MIN_I)
      RR_KIND(RR_MAX_I)
      RR_KIND(RR_MIN_F)
      RR_KIND(RR_MAX_F)
    }
#undef RR_KIND
  }
}

// ---------------------------------------------------------------------------
// host wrappers
//
// workspace layout for nb = ceil(n / tile) tiles and C columns, 8-byte
// aligned:
//   [scratch u64 x C*n][lead u64 x C*nb][base u64 x nb][heads u32 x nb]
// The caller fills base[] (exclusive scan of heads) between the two calls.

static inline uint32_t rr_tiles(uint32_t n) {
  return (uint32_t)(((uint64_t)n + RR_TILE - 1) / RR_TILE);
}

int reduce_records_tile() { return RR_TILE; }

int reduce_records_max_columns() { return RR_MAX_COLS; }

static void rr_check_ncols(int ncols) {
  if (ncols < 1 || ncols > RR_MAX_COLS)
    throw std::invalid_argument(
        "reduce_records: the column count must be in [1, 8]");
}

size_t reduce_records_workspace_bytes(uint32_t n, int ncols) {
  rr_check_ncols(ncols);
  const size_t nb = rr_tiles(n), c = (size_t)ncols;
  return c * n * 8 + c * nb * 8 + nb * 8 + ((nb * 4 + 7) & ~(size_t)7);
}

// rec_bytes == 0: the emit call, which reads no record (offsets unchecked)
static RrColumns rr_columns(const std::vector<uint32_t>& offs,
                            const std::vector<int>& types,
                            const std::vector<int>& ops, uint32_t rec_bytes) {
  rr_check_ncols((int)offs.size());
  if (types.size() != offs.size() || ops.size() != offs.size())
    throw std::invalid_argument("reduce_records: column lists differ in length");
  RrColumns cols{};
  for (size_t c = 0; c < offs.size(); ++c) {
    if (ops[c] < 0 || ops[c] > RR_COUNT)
      throw std::invalid_argument("reduce_records: unknown op code");
    if (ops[c] == RR_COUNT) {
      cols.c[c] = RrColumn{0, RR_I64, RR_COUNT};
      continue;
    }
    if (types[c] < 0 || types[c] > RR_F64)
      throw std::invalid_argument("reduce_records: unknown type code");
    const uint32_t size = types[c] == RR_I64 || types[c] == RR_F64 ? 8 : 4;
    if (offs[c] > 0xffffu ||
        (rec_bytes && (uint64_t)offs[c] * 4 + size > rec_bytes))
      throw std::invalid_argument(
          "reduce_records: a column reaches past the record");
    cols.c[c] = RrColumn{(uint16_t)offs[c], (uint8_t)types[c], (uint8_t)ops[c]};
  }
  return cols;
}

void reduce_records_count(uintptr_t pairs, uint32_t n, uintptr_t recs,
                          uint32_t rec_bytes, uintptr_t segs, uint32_t nsegs,
                          const std::vector<uint32_t>& col_words,
                          const std::vector<int>& col_types,
                          const std::vector<int>& col_ops, uintptr_t ws,
                          uintptr_t stream) {
  if (rec_bytes == 0 || rec_bytes % 4)
    throw std::invalid_argument(
        "reduce_records: rec_bytes must be a positive multiple of 4");
  const RrColumns cols = rr_columns(col_words, col_types, col_ops, rec_bytes);
  if (n == 0) return;
  if ((pairs & 15) || (ws & 7) || (recs & 3) || (segs & 7))
    throw std::invalid_argument("reduce_records: misaligned buffer");
  if (nsegs == 0 ? recs == 0 : segs == 0)
    throw std::invalid_argument("reduce_records: no record source");
  const uint32_t nb = rr_tiles(n), C = (uint32_t)col_words.size();
  auto* scratch = reinterpret_cast<uint64_t*>(ws);
  auto* lead = scratch + (size_t)C * n;
  auto* base = lead + (size_t)C * nb;
  auto* heads = reinterpret_cast<uint32_t*>(base + nb);
  hipLaunchKernelGGL((reduce_records_kernel<false>), dim3(nb), dim3(RR_BLOCK),
                     0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const ulonglong2*>(pairs), n,
                     reinterpret_cast<const uint32_t*>(recs),
                     reinterpret_cast<const RecSegment*>(segs), nsegs,
                     rec_bytes / 4, cols, C, scratch, heads, lead, base,
                     (uint64_t)0, (uint64_t*)nullptr, (uint64_t*)nullptr);
  HIP_CHECK(hipGetLastError());
}

void reduce_records_emit(uintptr_t pairs, uint32_t n,
                         const std::vector<int>& col_types,
                         const std::vector<int>& col_ops, uintptr_t ws,
                         uint64_t g, uintptr_t out_keys, uintptr_t out_vals,
                         uintptr_t stream) {
  const RrColumns cols = rr_columns(
      std::vector<uint32_t>(col_types.size(), 0), col_types, col_ops, 0);
  if (n == 0) return;
  if ((pairs & 15) || (ws & 7) || (out_keys & 7) || (out_vals & 7))
    throw std::invalid_argument("reduce_records: misaligned buffer");
  if (g == 0 || g > n || out_keys == 0 || out_vals == 0)
    throw std::invalid_argument("reduce_records: bad output extent");
  const uint32_t nb = rr_tiles(n), C = (uint32_t)col_types.size();
  auto* scratch = reinterpret_cast<uint64_t*>(ws);
  auto* lead = scratch + (size_t)C * n;
  auto* base = lead + (size_t)C * nb;
  auto* heads = reinterpret_cast<uint32_t*>(base + nb);
  hipLaunchKernelGGL((reduce_records_kernel<true>), dim3(nb), dim3(RR_BLOCK),
                     0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const ulonglong2*>(pairs), n,
                     (const uint32_t*)nullptr, (const RecSegment*)nullptr, 0u,
                     0u, cols, C, scratch, heads, lead, base, g,
                     reinterpret_cast<uint64_t*>(out_keys),
                     reinterpret_cast<uint64_t*>(out_vals));
  HIP_CHECK(hipGetLastError());
}

}  // namespace hipshuffle
