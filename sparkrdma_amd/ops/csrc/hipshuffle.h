// Public surface of the hipshuffle native library.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace hipshuffle {

// pool.cpp
int slab_alloc_id(size_t bytes);
void slab_free_id(int id);
uintptr_t slab_base_id(int id);
std::string slab_handle_id(int id);
uintptr_t ipc_open(const std::string& handle_bytes);
void ipc_close(uintptr_t ptr);
void enable_peer_access(int peer_device);
uint64_t read_batch_ids(int peer, const std::vector<uintptr_t>& dsts,
                        const std::vector<uintptr_t>& srcs,
                        const std::vector<size_t>& sizes);
// like read_batch_ids, but every (dst, src, size) is a run of whole
// rec_bytes-byte records moved by fetch_records, which also writes the
// run's (prefix, aux) pairs to pairs_ptrs[i] with indices from idx_bases[i]
uint64_t read_records_batch_ids(int peer, const std::vector<uintptr_t>& dsts,
                                const std::vector<uintptr_t>& srcs,
                                const std::vector<size_t>& sizes,
                                uint32_t rec_bytes, uint32_t key_bytes,
                                const std::vector<uintptr_t>& pairs_ptrs,
                                const std::vector<uint64_t>& idx_bases);
// the in-place counterpart: extract_records per (src, size), nothing is
// copied; same streams, same checks, one completion event
uint64_t extract_records_batch_ids(int peer,
                                   const std::vector<uintptr_t>& srcs,
                                   const std::vector<size_t>& sizes,
                                   uint32_t rec_bytes, uint32_t key_bytes,
                                   const std::vector<uintptr_t>& pairs_ptrs,
                                   const std::vector<uint64_t>& idx_bases);
bool poll_event(uint64_t id);
void wait_event(uint64_t id);
int64_t tcp_recv_chunks(int fd, uintptr_t out, uint64_t total);
int64_t tcp_send_all(int fd, uintptr_t buf, uint64_t n);
uintptr_t host_alloc_pinned(size_t n);
void host_free_pinned(uintptr_t p);
void memcpy_h2d(uintptr_t dst, uintptr_t src, size_t n);
void memcpy_d2h(uintptr_t dst, uintptr_t src, size_t n);

// kernels.hip
size_t radix_hist_bytes(uint32_t n, int nbits);
size_t radix_scan_ws_bytes(uint32_t n, int nbits);
void radix_hist(uintptr_t keys, uint32_t n, int shift, int nbits,
                uintptr_t hist, uintptr_t stream, int func = 0,
                int in_stride = 1, uint32_t nparts = 0);
void radix_scan(uintptr_t hist, uint32_t n, int nbits, uintptr_t totals,
                uintptr_t scan_ws, uintptr_t stream);
void radix_scatter(uintptr_t keys, uintptr_t vals, uint32_t n, int shift,
                   int nbits, uintptr_t hist, uintptr_t key_dst,
                   uintptr_t val_dst, uintptr_t stream, int func = 0,
                   int aos_out = 0, int in_stride = 1, uint32_t nparts = 0);
void extract_pairs(uintptr_t recs, uint64_t n, uint32_t rec_bytes,
                   uint32_t key_bytes, uintptr_t pairs, uintptr_t stream,
                   int pid_func = -1, int pid_shift = 0,
                   uint32_t pid_mask = 0, uint32_t pid_nparts = 0,
                   uint64_t idx_base = 0);
// segs / nsegs (here and in sort_records_u64 below): a device table of
// {u64 first_rec, const u32* base} entries sorted by first_rec and covering
// every record index; record idx is read at
// base[s] + (idx - first_rec[s]) * rec_bytes for the last s with
// first_rec[s] <= idx. nsegs == 0: contiguous from `recs`.
void gather_records(uintptr_t recs, uintptr_t pairs, uint64_t n,
                    uint32_t rec_bytes, int dst_mode, uint64_t out_base,
                    uintptr_t dst_addr, uintptr_t dstart, int shift,
                    uint32_t mask, int func, uint32_t nparts,
                    uintptr_t stream, uintptr_t segs = 0,
                    uint32_t nsegs = 0);
uint32_t fetch_block_records(uint32_t rec_bytes);
void fetch_records(uintptr_t dst, uintptr_t src, uint64_t n,
                   uint32_t rec_bytes, uint32_t key_bytes, uintptr_t pairs,
                   uint64_t idx_base, uintptr_t stream);
// fetch_records without the copy: the pairs of the n records at src, which
// stay where they are
void extract_records(uintptr_t src, uint64_t n, uint32_t rec_bytes,
                     uint32_t key_bytes, uintptr_t pairs, uint64_t idx_base,
                     uintptr_t stream);
size_t sort_workspace_bytes(uint32_t n);
int sort_pairs_u64(uintptr_t keys, uintptr_t vals, uintptr_t tmp_keys,
                   uintptr_t tmp_vals, uint32_t n, int start_bit, int end_bit,
                   uintptr_t ws, uintptr_t stream);
void probe_scatter_write(uintptr_t out, uint64_t region_elems,
                         uint32_t nregions, uint32_t burst_elems,
                         uint32_t bursts_per_block, uint32_t grid,
                         uintptr_t stream);
void join_count(uintptr_t a_keys, uint32_t na, uintptr_t b_keys,
                uint32_t nb_, uintptr_t counts, uintptr_t lo_idx,
                uintptr_t stream);
void join_emit(uintptr_t a_keys, uintptr_t a_vals, uint32_t na,
               uintptr_t b_vals, uintptr_t counts, uintptr_t lo_idx,
               uintptr_t offsets, uintptr_t out_key, uintptr_t out_a,
               uintptr_t out_b, uintptr_t stream);
size_t onesweep_workspace_bytes(uint32_t n, int passes);
void set_timing_buf(uintptr_t p);
// sort_word: the u64 of each 16-byte pair whose bits order the pairs
int onesweep_sort_aos_u64(uintptr_t pairs, uintptr_t tmp_pairs, uint32_t n,
                          int start_bit, int end_bit, uintptr_t ws,
                          uintptr_t stream, int sort_word = 0);
// Wide-record sort (kernels.hip): the extracted pairs in, the sorted records
// in `out`, always. Returns the path taken, as last_sort_path() reports it:
// 0 full pass sequence, 1 truncated sort with tie repair, 2 truncated, then
// full because a tied run was too long. Blocks on the stream once when a
// truncated attempt ran (paths 1 and 2), else never.
int sort_records_u64(uintptr_t pairs, uintptr_t tmp_pairs, uint32_t n,
                     int end_bit, int key_bytes, uintptr_t ws,
                     uintptr_t stream, uintptr_t recs, uintptr_t out,
                     uint32_t rec_bytes, int fuse = 1, uintptr_t segs = 0,
                     uint32_t nsegs = 0);
// bytes of its ws, whichever path it takes
size_t sort_records_workspace_bytes(uint32_t n, int end_bit, int key_bytes);
// Map-side partition of wide records by a digit of at most 8 bits, which
// pair.x holds (the partition id). count_pair_digits: totals u32[256] = how
// many of the n pairs have each id. partition_records_fused: record
// pair.y & (2^48 - 1) of `recs` goes to dst_table[pair.x] (device u64[256],
// 4-byte-aligned byte addresses; entries of empty partitions are never
// dereferenced) behind the same partition's earlier records, in one pass.
void count_pair_digits(uintptr_t pairs, uint32_t n, uintptr_t totals,
                       uintptr_t stream);
size_t partition_records_workspace_bytes(uint32_t n);
void partition_records_fused(uintptr_t pairs, uint32_t n, uintptr_t recs,
                             uint32_t rec_bytes, uintptr_t dst_table,
                             uintptr_t ws, uintptr_t stream);
void set_tie_repair(int m);
int last_sort_path();
int tie_repair_tile();
int tie_repair_max_run();
void sort_records_plan(uint32_t n, int end_bit, int* lo_bit, int* passes,
                       int* run_bits);
int onesweep_sort_pairs_u64(uintptr_t keys, uintptr_t vals,
                            uintptr_t tmp_keys, uintptr_t tmp_vals,
                            uint32_t n, int start_bit, int end_bit,
                            uintptr_t ws, uintptr_t stream);

// reduce.hip — segmented reduce over key-sorted AoS (key, value) pairs.
// op: 0 sum (i64, wraps), 1 sum_f64, 2 count, 3 min (i64), 4 max (i64).
// Workspace: [lead u64 x nb][base u64 x nb][heads u32 x nb] for
// nb = ceil(n / tile); the caller writes base[] = exclusive scan of heads[]
// between the count and the emit call, and sizes out_* from its total.
int reduce_by_key_tile();
size_t reduce_by_key_workspace_bytes(uint32_t n);
void reduce_by_key_count(uintptr_t pairs, uint32_t n, int op, uintptr_t ws,
                         uintptr_t stream);
void reduce_by_key_emit(uintptr_t pairs, uint32_t n, int op, uintptr_t ws,
                        uintptr_t out_keys, uintptr_t out_vals,
                        uintptr_t stream);

// reduce_records.hip — segmented reduce of 1..8 typed columns of W-byte
// records over key-sorted (key, aux) pairs; record index = aux & (2^48 - 1),
// the records contiguous at `recs` or behind the segs / nsegs table of
// gather_records. Column c is (col_words[c] = offset / 4, col_types[c]:
// 0 i32, 1 u32, 2 i64, 3 f32, 4 f64, col_ops[c]: 0 sum, 1 min, 2 max,
// 3 count — offset and type ignored). Integers reduce as i64, floats as f64.
// Workspace: [scratch u64 x C*n][lead u64 x C*nb][base u64 x nb]
// [heads u32 x nb] for nb = ceil(n / tile); the caller writes base[] =
// exclusive scan of heads[] between the count and the emit call, g = their
// total. Output: out_keys u64[g], column c at out_vals + c * g.
int reduce_records_tile();
int reduce_records_max_columns();
size_t reduce_records_workspace_bytes(uint32_t n, int ncols);
void reduce_records_count(uintptr_t pairs, uint32_t n, uintptr_t recs,
                          uint32_t rec_bytes, uintptr_t segs, uint32_t nsegs,
                          const std::vector<uint32_t>& col_words,
                          const std::vector<int>& col_types,
                          const std::vector<int>& col_ops, uintptr_t ws,
                          uintptr_t stream);
void reduce_records_emit(uintptr_t pairs, uint32_t n,
                         const std::vector<int>& col_types,
                         const std::vector<int>& col_ops, uintptr_t ws,
                         uint64_t g, uintptr_t out_keys, uintptr_t out_vals,
                         uintptr_t stream);

// bounds.hip — pair extraction with the partition id in pair.x, found by
// searching `nbounds` ascending u64 split points (device memory):
// x = #{bounds <= key prefix}, unsigned; aux as extract_pairs writes it.
void extract_pairs_bounds(uintptr_t recs, uint64_t n, uint32_t rec_bytes,
                          uint32_t key_bytes, uintptr_t pairs,
                          uintptr_t bounds, uint32_t nbounds,
                          uintptr_t stream, uint64_t idx_base = 0);

// join.hip — sort-merge join family over key-sorted SoA tables; P probes Q,
// keys compare as unsigned 64-bit, np and nq < 2^31.
// join_probe: lo[i] = lower_bound(Q, pkey[i]), m[i] = matches of row i (u32).
// join_expand: output row o belongs to the last P row i with
// offsets[i] <= o (offsets: exclusive u64 scan of the per-row output
// counts, total: their sum) and is its match j = o - offsets[i]. Every
// out_* may be 0 (skipped): out_key / out_p_val / out_p_idx take pkey[i],
// pval[i], i; out_q_val / out_q_valid (u8) / out_q_idx (i64) take
// qval[lo[i] + j], 1, lo[i] + j where m[i] != 0 and 0, 0, -1 elsewhere.
int join_expand_tile();
int join_expand_lds_rows();
int join_probe_lds_keys();
void join_probe(uintptr_t p_keys, uint32_t np, uintptr_t q_keys, uint32_t nq,
                uintptr_t lo, uintptr_t m, uintptr_t stream);
void join_expand(uintptr_t p_keys, uintptr_t p_vals, uintptr_t q_vals,
                 uintptr_t lo, uintptr_t m, uintptr_t offsets, uint32_t np,
                 uint64_t total, uintptr_t out_key, uintptr_t out_p_val,
                 uintptr_t out_q_val, uintptr_t out_q_valid,
                 uintptr_t out_p_idx, uintptr_t out_q_idx,
                 uintptr_t stream);

// varlen.hip — byte-granular copy of n rows of different lengths, balanced
// by destination bytes. cum: u64[n + 1] exclusive scan of the row lengths in
// destination order (cum[0] == 0, cum[n] == total); src: u64[n] byte address
// of every row; the destination is nseg contiguous ranges: range s takes the
// virtual bytes [seg_off[s], seg_off[s + 1]) (u64[nseg + 1], seg_off[0] == 0,
// seg_off[nseg] == total) at byte address seg_dst[s] (u64[nseg]). Any source
// and destination alignment; no byte outside a range is written.
// n, nseg < 2^31. wide_loads == 0 reads every source byte with a byte load
// (the measured alternative, scripts/bench_varlen.py).
int varlen_copy_tile_bytes();
int varlen_copy_lds_rows();
void varlen_copy(uintptr_t cum, uintptr_t src, uint64_t n, uintptr_t seg_off,
                 uintptr_t seg_dst, uint64_t nseg, uint64_t total,
                 uintptr_t stream, int wide_loads = 1);

}  // namespace hipshuffle
