// Byte-granular copy of many rows of different lengths for MI355X (gfx950):
// the data mover of the variable-length record lane (sparkrdma_amd/varlen.py
// has the wire format). It is the byte-level cousin of join_expand_kernel:
// OUTPUT-centric, an owner search over scanned offsets, and no thread's work
// depends on a row's length.
//
// Inputs
//   cum[n + 1]      exclusive u64 scan of the row lengths in DESTINATION
//                   order, cum[0] == 0; total = cum[n]
//   src[n]          device byte address of every row's first byte, any
//                   alignment (never read for a row of length 0)
//   seg_off[S + 1]  the destination is S contiguous ranges; range s takes
//                   the virtual bytes [seg_off[s], seg_off[s + 1]) — that is
//                   cum[seg_first_row[s]], gathered by the caller — with
//                   seg_off[0] == 0 and seg_off[S] == total
//   seg_dst[S]      device byte address of every range, any alignment
//                   (never read for an empty range)
//
// Decomposition. The virtual byte range [0, total) is cut into tiles of
// VARLEN_TILE bytes, one block each, and a tile into 16-byte grid intervals,
// VARLEN_ITEMS per thread. The unit of work is a PIECE: the part of one
// 16-byte-ALIGNED destination granule that lies inside one range. A piece
// belongs to the grid interval that holds its first byte, so every
// destination byte is written exactly once, by exactly one thread. A grid
// interval owns at most one piece that starts on a granule edge plus one per
// range that starts inside it: <= 17 pieces, each <= 16 bytes.
//
//   piece of 16 bytes   granule-aligned, wholly inside its range: ONE
//                       16-byte store. It may hold the bytes of several
//                       short rows — the destination is contiguous inside a
//                       range.
//   shorter piece       only the first and last granule of a range are cut
//                       short: byte stores of exactly the bytes inside the
//                       range. No store touches a byte outside a range.
//
// A piece may reach up to 15 bytes into the next tile's virtual bytes, so a
// block's row window covers [tile0, tile0 + VARLEN_TILE + 15).
//
// Owner lookup. Four waves find, with one wave_count_below each, the rows
// that own the window's first and last byte and the ranges that hold them.
// A window of at most VARLEN_LDS_ROWS rows has its row offsets staged in LDS
// as u32 relative to tile0 (clamped at both ends: only the first row can
// start before the tile, only the last can end after the window; the first
// row's true start is kept for the source offset). A window of more rows —
// thousands of 0- or 1-byte rows — is searched in global memory. Both
// searches take the LAST row with start <= byte: rows of length 0 share
// their start with the next row and are never chosen. The ranges of a
// window are searched in global memory; there are rarely more than two.
//
// Source bytes. A full piece whose 16 bytes come from one row is read with
// two 16-byte-aligned loads and a byte shift (one load when the source is
// aligned). Each aligned load covers at least one byte of the row, so it
// stays inside the row's 16-byte granules. Every other piece is assembled
// from byte loads and changes row as often as it must: at most 16 bytes, so
// at most 16 steps, whatever the rows' lengths.
//
// A row longer than a tile is simply the owner of every piece of many
// blocks. No loop is bounded by a row length, no atomics, no block waits on
// another block, plain vector stores only. Limits: n, S < 2^31; offsets and
// totals are 64-bit.

#include "common.h"
#include "hipshuffle.h"

#include <hip/hip_runtime.h>

namespace hipshuffle {

constexpr int VARLEN_BLOCK = 256;
constexpr int VARLEN_ITEMS = 4;
constexpr uint32_t VARLEN_GRAIN = 16;                       // store width
constexpr uint32_t VARLEN_TILE = VARLEN_BLOCK * VARLEN_ITEMS * VARLEN_GRAIN;
constexpr uint32_t VARLEN_LDS_ROWS = 4096;                  // 16 KB of u32
constexpr uint32_t VARLEN_REL_CAP = VARLEN_TILE + VARLEN_GRAIN;
constexpr uint64_t VARLEN_MAX_ROWS = 0x7fffffffull;

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) {
  return a < b ? a : b;
}

struct VarlenArgs {
  const uint64_t* cum;
  const uint64_t* src;
  const uint64_t* seg_off;
  const uint64_t* seg_dst;
  uint32_t n;
  uint32_t nseg;
  uint64_t total;
};

// The rows [i0, i0 + cnt) of one block's window; `cum` and `src` point at
// row i0. LDS: rel[r] = start of row r relative to tile0 for r <= cnt,
// rel[0] == 0 and rel[cnt] <= VARLEN_REL_CAP by clamping.
template <bool LDS>
struct RowWindow {
  const uint64_t* cum;
  const uint64_t* src;
  const uint32_t* rel;
  uint32_t cnt;
  uint64_t tile0;
  uint64_t off0;          // true start of row 0

  // the last row whose start is <= virtual byte p (p inside the window)
  __device__ __forceinline__ uint32_t owner(uint64_t p) const {
    uint32_t lo = 0, hi = cnt;
    if (LDS) {
      const uint32_t x = (uint32_t)(p - tile0);
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rel[mid] <= x) lo = mid + 1; else hi = mid;
      }
    } else {
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] <= p) lo = mid + 1; else hi = mid;
      }
    }
    return lo - 1;
  }
  __device__ __forceinline__ uint64_t start(uint32_t r) const {
    if (LDS) return r ? tile0 + rel[r] : off0;
    return cum[r];
  }
  // exact up to the window's end, clamped beyond it (LDS)
  __device__ __forceinline__ uint64_t end(uint32_t r) const {
    if (LDS) return tile0 + rel[r + 1];
    return cum[r + 1];
  }
  __device__ __forceinline__ const uint8_t* at(uint32_t r, uint64_t p) const {
    return reinterpret_cast<const uint8_t*>(src[r]) + (p - start(r));
  }
};

// the 16 bytes at s, any alignment, from the aligned granules that hold them
__device__ __forceinline__ void load16_shift(const uint8_t* s, uint64_t* lo,
                                             uint64_t* hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s) & ~(uintptr_t)15;
  const uint32_t sh = ((uint32_t)reinterpret_cast<uintptr_t>(s) & 15u) * 8;
  const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(a);
  if (sh == 0) {
    *lo = v0.x;
    *hi = v0.y;
    return;
  }
  const ulonglong2 v1 = *reinterpret_cast<const ulonglong2*>(a + 16);
  if (sh < 64) {
    *lo = (v0.x >> sh) | (v0.y << (64 - sh));
    *hi = (v0.y >> sh) | (v1.x << (64 - sh));
  } else if (sh == 64) {
    *lo = v0.y;
    *hi = v1.x;
  } else {
    const uint32_t k = sh - 64;
    *lo = (v0.y >> k) | (v1.x << (64 - k));
    *hi = (v1.x >> k) | (v1.y << (64 - k));
  }
}

// virtual bytes [p, p + len) -> d, 1 <= len <= 16; d is 16-byte aligned when
// len == 16
template <bool LDS, bool WIDE>
__device__ __forceinline__ void copy_piece(const RowWindow<LDS>& w,
                                           uint64_t p, uint32_t len,
                                           uint8_t* d) {
  uint32_t r = w.owner(p);
  uint64_t re = w.end(r);
  const uint8_t* s = w.at(r, p);
  uint64_t lo = 0, hi = 0;
  if (WIDE && len == VARLEN_GRAIN && re - p >= VARLEN_GRAIN) {
    load16_shift(s, &lo, &hi);
  } else {
    uint64_t q = p;
#pragma unroll 1
    for (uint32_t k = 0; k < len; ++k, ++q, ++s) {
      if (q >= re) {
        // the next row with a byte: usually r + 1, else search past the
        // rows of length 0
        ++r;
        if (w.end(r) <= q) r = w.owner(q);
        re = w.end(r);
        s = w.at(r, q);
      }
      const uint64_t b = *s;
      if (k < 8) lo |= b << (8 * k); else hi |= b << (8 * (k - 8));
    }
  }
  if (len == VARLEN_GRAIN) {
    *reinterpret_cast<ulonglong2*>(d) = make_ulonglong2(lo, hi);
  } else {
#pragma unroll 1
    for (uint32_t k = 0; k < len; ++k)
      d[k] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
  }
}

// the grid intervals of one tile; ranges [s0, s0 + scnt) hold its bytes
template <bool LDS, bool WIDE>
__device__ __forceinline__ void varlen_tile(const VarlenArgs& a,
                                            const RowWindow<LDS>& w,
                                            uint64_t tile0, uint32_t s0,
                                            uint32_t scnt, uint32_t t) {
  const uint64_t* __restrict__ soff = a.seg_off + s0;
  const uint64_t* __restrict__ sdst = a.seg_dst + s0;
  if (scnt == 1 && ((sdst[0] - soff[0]) & (VARLEN_GRAIN - 1)) == 0) {
    // ONE range holds the whole window and its granules lie on the grid
    // (tile0 is a multiple of 16): interval g IS the piece at g. The
    // common case — every segment of the shuffle lanes starts 16-byte
    // aligned at a multiple of 16 virtual bytes. Straight-line phases, so
    // that the VARLEN_ITEMS source loads of a thread are in flight
    // together: owner search (LDS), row address, 16-byte loads, stores. A
    // piece that is cut short or spans rows takes copy_piece.
    const uint64_t rs = soff[0], re = soff[1], base = sdst[0];
    uint32_t r[VARLEN_ITEMS];
    bool fast[VARLEN_ITEMS];
    const uint8_t* src[VARLEN_ITEMS];
    uint64_t lo[VARLEN_ITEMS], hi[VARLEN_ITEMS];
#pragma unroll
    for (int it = 0; it < VARLEN_ITEMS; ++it) {
      const uint64_t g =
          tile0 + (uint64_t)(it * VARLEN_BLOCK + t) * VARLEN_GRAIN;
      fast[it] = false;
      if (WIDE && g + VARLEN_GRAIN <= re) {
        r[it] = w.owner(g);
        fast[it] = w.end(r[it]) - g >= VARLEN_GRAIN;
      }
    }
#pragma unroll
    for (int it = 0; it < VARLEN_ITEMS; ++it) {
      const uint64_t g =
          tile0 + (uint64_t)(it * VARLEN_BLOCK + t) * VARLEN_GRAIN;
      if (fast[it]) src[it] = w.at(r[it], g);
    }
#pragma unroll
    for (int it = 0; it < VARLEN_ITEMS; ++it)
      if (fast[it]) load16_shift(src[it], &lo[it], &hi[it]);
#pragma unroll
    for (int it = 0; it < VARLEN_ITEMS; ++it) {
      const uint64_t g =
          tile0 + (uint64_t)(it * VARLEN_BLOCK + t) * VARLEN_GRAIN;
      uint8_t* d = reinterpret_cast<uint8_t*>(base + (g - rs));
      if (fast[it])
        *reinterpret_cast<ulonglong2*>(d) = make_ulonglong2(lo[it], hi[it]);
      else if (g < re)
        copy_piece<LDS, WIDE>(
            w, g, (uint32_t)min64(VARLEN_GRAIN, re - g), d);
    }
    return;
  }
  uint64_t rs = 0, re = 0, base = 0;      // the range that holds p; p only
                                          // grows, so it is kept across items
#pragma unroll 1
  for (int it = 0; it < VARLEN_ITEMS; ++it) {
    const uint64_t g =
        tile0 + (uint64_t)(it * VARLEN_BLOCK + t) * VARLEN_GRAIN;
    if (g >= a.total) break;
    const uint64_t gend = min64(g + VARLEN_GRAIN, a.total);
    uint64_t p = g;
    while (p < gend) {                    // <= 18 rounds, see the header
      if (p >= re) {
        // the LAST range that starts at or before p: empty ranges share
        // their start with the next one and are never chosen
        uint32_t lo = 0, hi = scnt;
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (soff[mid] <= p) lo = mid + 1; else hi = mid;
        }
        rs = soff[lo - 1];
        re = soff[lo];
        base = sdst[lo - 1];
      }
      const uint64_t d = base + (p - rs);
      const uint32_t k = (uint32_t)d & (VARLEN_GRAIN - 1);
      const uint64_t pe = min64(p + (VARLEN_GRAIN - k), re);
      // p opens a piece when it starts a granule or a range; any other p is
      // the interval's first byte inside a piece of the interval before
      if (k == 0 || p == rs)
        copy_piece<LDS, WIDE>(w, p, (uint32_t)(pe - p),
                              reinterpret_cast<uint8_t*>(d));
      p = pe;
    }
  }
}

template <bool WIDE>
__global__ __launch_bounds__(VARLEN_BLOCK) void varlen_copy_kernel(
    const VarlenArgs a) {
  __shared__ uint32_t s_rel[VARLEN_LDS_ROWS + 1];
  __shared__ uint32_t s_rng[4];
  const uint32_t t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * VARLEN_TILE;  // < total
  const uint64_t wend = min64(tile0 + VARLEN_REL_CAP - 1, a.total);

  // owners of the window's first and last byte (waves 0, 1: rows; 2, 3:
  // ranges). cum[0] == seg_off[0] == 0 <= any byte: the counts are >= 1
  {
    const uint32_t wv = t / kWave, lane = t & (kWave - 1);
    const uint64_t p = (wv & 1) ? wend - 1 : tile0;
    const uint32_t c = wv < 2
        ? wave_count_below<false>(a.cum, a.n, p, lane)
        : wave_count_below<false>(a.seg_off, a.nseg, p, lane);
    if (lane == 0) s_rng[wv] = c - 1;
  }
  __syncthreads();
  const uint32_t i0 = s_rng[0];
  const uint32_t cnt = s_rng[1] - i0 + 1;          // block-uniform
  const uint32_t s0 = s_rng[2];
  const uint32_t scnt = s_rng[3] - s0 + 1;

  if (cnt <= VARLEN_LDS_ROWS) {
    // cum[i0] <= tile0 < cum[i0 + r] < wend for 1 <= r < cnt; cum[i0 + cnt]
    // >= wend is clamped: it is only compared with bytes inside the window
    for (uint32_t r = t; r <= cnt; r += VARLEN_BLOCK) {
      const uint64_t c = a.cum[i0 + r];
      s_rel[r] = c <= tile0 ? 0u
               : (uint32_t)min64(c - tile0, VARLEN_REL_CAP);
    }
    __syncthreads();
    const RowWindow<true> w{a.cum + i0, a.src + i0, s_rel, cnt, tile0,
                            a.cum[i0]};
    varlen_tile<true, WIDE>(a, w, tile0, s0, scnt, t);
  } else {
    const RowWindow<false> w{a.cum + i0, a.src + i0, nullptr, cnt, tile0, 0};
    varlen_tile<false, WIDE>(a, w, tile0, s0, scnt, t);
  }
}

// ---------------------------------------------------------------------------
// host wrapper

int varlen_copy_tile_bytes() { return (int)VARLEN_TILE; }
int varlen_copy_lds_rows() { return (int)VARLEN_LDS_ROWS; }

void varlen_copy(uintptr_t cum, uintptr_t src, uint64_t n, uintptr_t seg_off,
                 uintptr_t seg_dst, uint64_t nseg, uint64_t total,
                 uintptr_t stream, int wide_loads) {
  if (n > VARLEN_MAX_ROWS)
    throw std::invalid_argument("varlen_copy: row count exceeds 2^31 - 1");
  if (nseg > VARLEN_MAX_ROWS)
    throw std::invalid_argument("varlen_copy: range count exceeds 2^31 - 1");
  if (total == 0) return;
  if (n == 0 || nseg == 0)
    throw std::invalid_argument("varlen_copy: bytes to copy but no row or "
                                "no destination range");
  const uint64_t grid = (total + VARLEN_TILE - 1) / VARLEN_TILE;
  if (grid > 0x7fffffffull)
    throw std::invalid_argument("varlen_copy: total exceeds the grid limit");
  if (!cum || !src || !seg_off || !seg_dst)
    throw std::invalid_argument("varlen_copy: null table");
  if ((cum | src | seg_off | seg_dst) & 7)
    throw std::invalid_argument("varlen_copy: misaligned table");
  VarlenArgs a;
  a.cum = reinterpret_cast<const uint64_t*>(cum);
  a.src = reinterpret_cast<const uint64_t*>(src);
  a.seg_off = reinterpret_cast<const uint64_t*>(seg_off);
  a.seg_dst = reinterpret_cast<const uint64_t*>(seg_dst);
  a.n = (uint32_t)n;
  a.nseg = (uint32_t)nseg;
  a.total = total;
  if (wide_loads)
    hipLaunchKernelGGL(varlen_copy_kernel<true>, dim3((uint32_t)grid),
                       dim3(VARLEN_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(varlen_copy_kernel<false>, dim3((uint32_t)grid),
                       dim3(VARLEN_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace hipshuffle
