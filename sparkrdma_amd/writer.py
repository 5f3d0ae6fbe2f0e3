"""Shuffle write path.

Re-design of the reference write path (RdmaWrapperShuffleWriter.scala +
RdmaMappedFile.java). The reference delegates record partitioning to
Spark's CPU sort-shuffle writers, then mmaps + registers the resulting
data file and fills a per-partition (addr, len, key) table
(RdmaMappedFile.java:113-157). The MI355X design removes the file from the
fast path entirely: partitioned bytes are laid out directly in pool blocks
(host shm now; HBM slabs via the GPU writer in ops/), the table is filled
from the layout, and publishing is a one-sided 12-byte write.

Block chunking keeps the reference policy (RdmaMappedFile.java:113-157):
partitions are packed greedily into ~shuffle_write_block_size blocks, split
only at partition boundaries, so every partition is one contiguous
(addr, len) range. ``group_partitions`` is that policy for all three
lanes; the two GPU lanes (16-byte direct scatter, wide-record gather)
share one placement and publication step, ``_GpuLayout``, and differ only
in the kernels that write to the addresses it hands out.

Record model (fixed-width path): a partition segment is AoS —
``[key u64 | value bytes] × n`` interleaved records (doubles the GPU
scatter's per-digit write bursts and lets the reduce side consume fetched
chunks without splitting); n is inferable from the segment length. The
bytes path (arbitrary pickled records) concatenates pickle frames.
Variable-length rows (u64 key + payload of any length; ``write_varlen``,
``write_device_varlen``) have the segment format of ``varlen.py``: a
header, a (key, end) index and a payload heap per partition, placed by the
same ``_GpuLayout`` and written by one byte-balanced copy
(ops/csrc/varlen.hip).
"""

from __future__ import annotations

import pickle
import time
from typing import List, Optional

import numpy as np

from .manager import ShuffleHandle, ShuffleManager
from .map_output import make_key
from .partitioner import GPU_PART_BOUNDS as PART_BOUNDS
from .stats import TaskMetrics

HEADER_W = 8  # bytes per key


def pack_partition_segment(keys: np.ndarray, values: Optional[np.ndarray]) -> bytes:
    """AoS record layout: [key u64 | value bytes] interleaved per record.

    Interleaving doubles the GPU scatter's per-digit write-burst length
    (the partition kernel writes the identical layout) and lets the
    reduce side consume fetched chunks without a split/concat step.
    """
    if values is None or values.size == 0:
        return keys.astype("<u8", copy=False).tobytes()
    n = len(keys)
    vw = values.shape[1]
    rec = np.empty((n, HEADER_W + vw), dtype=np.uint8)
    rec[:, :HEADER_W] = keys.astype("<u8", copy=False).view(np.uint8).reshape(n, 8)
    rec[:, HEADER_W:] = values
    return rec.tobytes()


def unpack_partition_segment(buf, value_width: int):
    if value_width == 0:
        return np.frombuffer(buf, dtype="<u8"), None
    rec_w = HEADER_W + value_width
    n = len(buf) // rec_w
    arr = np.frombuffer(buf, dtype=np.uint8)[:n * rec_w].reshape(n, rec_w)
    keys = arr[:, :HEADER_W].copy().view("<u8").reshape(n)
    values = arr[:, HEADER_W:]
    return keys, values


def group_partitions(seg_bytes, write_block: int) -> List[List[int]]:
    """The block policy of every lane: partitions are taken in order and a
    group (one pool block) is closed before the partition that would push
    it past ``write_block``. A group is never empty, so a partition larger
    than ``write_block`` is a group of its own."""
    groups: List[List[int]] = []
    group: List[int] = []
    group_bytes = 0
    for p, nb in enumerate(seg_bytes):
        if group and group_bytes + nb > write_block:
            groups.append(group)
            group, group_bytes = [], 0
        group.append(p)
        group_bytes += int(nb)
    if group:
        groups.append(group)
    return groups


class _GpuLayout:
    """Where a GPU lane's kernel writes each partition of one map output.

    Construction places the groups of ``seg_bytes`` (int64 bytes per
    partition) in HBM pool blocks and fills the location table. A group
    the pool cannot serve spills (the reference keeps a disk file path for
    overflow — SURVEY §7.1 RdmaMappedFile row): its partitions go to one
    transient device staging tensor, and ``finish`` copies them to a host
    pool block. ``dst`` (int64[nd], the table the kernel indexes by digit)
    holds the device byte address of every non-empty partition, in HBM or
    in the staging tensor; 0 for empty partitions and digits >= R."""

    def __init__(self, writer: "ShuffleWriter", seg_bytes: np.ndarray,
                 nd: int, device):
        import torch
        mgr = writer.manager
        self.writer, self.seg_bytes = writer, seg_bytes
        self.table, self.table_addr = mgr.alloc_table(
            len(seg_bytes), writer.handle.shuffle_id)
        self.blocks = []
        self.dst = np.zeros(nd, dtype=np.int64)
        self.spilled = []   # (parts, total) that did not fit the HBM pool
        meta_key = make_key(mgr.executor_id, 1)
        for parts in group_partitions(seg_bytes,
                                      mgr.conf.shuffle_write_block_size):
            total = int(sum(seg_bytes[p] for p in parts))
            if total == 0:
                for p in parts:
                    self.table.put(p, 0, 0, meta_key)
                continue
            try:
                blk = mgr.gpu.pool.get(total)
            except MemoryError:
                self.spilled.append((parts, total))
                continue
            self._put(parts, blk.offset,
                      make_key(mgr.executor_id, blk.segment_id),
                      mgr.gpu.local_base(blk.segment_id))
            self.blocks.append(blk)
        self.stage = torch.empty(sum(t for _, t in self.spilled),
                                 dtype=torch.uint8, device=device)
        addr = self.stage.data_ptr()
        for parts, _total in self.spilled:
            for p in parts:
                if seg_bytes[p]:
                    self.dst[p] = addr
                addr += int(seg_bytes[p])

    def _put(self, parts, off: int, key: int, base: Optional[int] = None):
        """Table entries of one placed group, back to back from offset
        ``off`` of its segment; for an HBM block ``base``, the slab's
        device address, also sets ``dst``."""
        for p in parts:
            nb = int(self.seg_bytes[p])
            self.table.put(p, off, nb, key)
            if nb and base is not None:
                self.dst[p] = base + off
            off += nb
            self.writer.metrics.bytes_written += nb

    def finish(self, records: int) -> None:
        """After the kernel is queued: wait for it, move the spilled groups
        to host blocks, publish."""
        import torch
        w = self.writer
        mgr = w.manager
        torch.cuda.synchronize()
        soff = 0
        for parts, total in self.spilled:
            hblk = mgr.pool.get(total)     # host pool
            mgr.data_segment(hblk.segment_id).write(
                hblk.offset,
                self.stage[soff:soff + total].cpu().numpy().tobytes())
            self._put(parts, hblk.offset,
                      make_key(mgr.executor_id, hblk.segment_id))
            soff += total
            self.blocks.append(hblk)
        w.metrics.records_written += records
        mgr.keep_alive(w.handle, w.map_id, self.blocks)
        mgr.publish_map_output(w.handle, w.map_id, self.table_addr)


class ShuffleWriter:
    """One map task's writer: accumulate → partition → lay out → publish."""

    def __init__(self, manager: ShuffleManager, handle: ShuffleHandle, map_id: int):
        self.manager = manager
        self.handle = handle
        self.map_id = map_id
        self.metrics = TaskMetrics()
        self._key_batches: List[np.ndarray] = []
        self._value_batches: List[Optional[np.ndarray]] = []
        self._byte_records: Optional[List[List[bytes]]] = None
        self._gpu_batches: list = []      # (keys, values) device tensors
        self._gpu_records: list = []      # flat uint8 device tensors
        self._record_shape: Optional[tuple] = None  # (record, key) bytes
        self._varlen_batches: list = []   # (keys, offsets, data) numpy
        self._gpu_varlen: list = []       # (keys, offsets, data) device
        self._stopped = False

    # -- fixed-width tensor path ---------------------------------------

    def write_batch(self, keys: np.ndarray, values: Optional[np.ndarray] = None) -> None:
        if values is not None and len(values) != len(keys):
            raise ValueError("keys/values length mismatch")
        self._check_lane("write_batch")
        self._key_batches.append(np.ascontiguousarray(keys, dtype=np.uint64))
        self._value_batches.append(
            None if values is None else np.ascontiguousarray(values, dtype=np.uint8))

    # -- GPU tensor path: CDNA4 partition kernel into HBM blocks --------

    def write_device_batch(self, keys, values=None) -> None:
        """keys/values: int64 CUDA tensors. Partitioned and serialized by
        the radix kernel straight into HBM pool blocks at stop()."""
        self._check_lane("write_device_batch")
        self._gpu_batches.append((keys, values))

    def write_device_records(self, records, record_bytes: int,
                             key_bytes: int = 8) -> None:
        """Wide-record GPU path (canonical TeraSort: 100-byte records =
        10 B key + 90 B value). ``records`` is a flat uint8 CUDA tensor of
        n*record_bytes; key layout: u64 LE prefix at offset 0 (+ u16 LE
        low bits at offset 8 when key_bytes == 10). The reference's
        contract is 'serve whatever bytes the writer produced'
        (RdmaMappedFile.java:113-157) — this is the GPU fast path for it
        (r01 handled only 16-byte records)."""
        if record_bytes % 4 or record_bytes < 8:
            raise ValueError("record_bytes must be a multiple of 4, >= 8")
        if key_bytes not in (8, 10):
            raise ValueError("key_bytes must be 8 or 10")
        if records.numel() % record_bytes:
            raise ValueError("records length not a record multiple")
        prev = self._record_shape
        if prev is not None and prev != (record_bytes, key_bytes):
            raise ValueError("record shape changed between batches")
        self._check_lane("write_device_records")
        self._record_shape = (record_bytes, key_bytes)
        self._gpu_records.append(records)

    # -- arbitrary-record path -----------------------------------------

    def write_records(self, records, partitioner=None) -> None:
        """records: iterable of (key, value) python objects. Partition by
        ``partitioner`` when given (a callable key->pid, or an object with
        ``partition_ids`` for integer keys); default is pickled-key crc32
        (stable across processes)."""
        R = self.handle.num_partitions
        self._check_lane("write_records")
        if self._byte_records is None:
            self._byte_records = [[] for _ in range(R)]
        import zlib
        if partitioner is None:
            def pid_of(k):
                return zlib.crc32(pickle.dumps(k, protocol=4)) % R
        elif hasattr(partitioner, "partition_ids"):
            def pid_of(k):
                return int(partitioner.partition_ids(
                    np.array([k], dtype=np.uint64))[0])
        elif callable(partitioner):
            def pid_of(k):
                return int(partitioner(k)) % R
        else:
            raise TypeError(f"unsupported partitioner {partitioner!r}")
        for k, v in records:
            pid = pid_of(k)
            if not 0 <= pid < R:
                raise ValueError(f"partitioner returned {pid} for key {k!r}, "
                                 f"outside [0, {R})")
            self._byte_records[pid].append(pickle.dumps((k, v), protocol=4))
            self.metrics.records_written += 1

    # -- variable-length rows (varlen.py has the wire format) -----------

    def _check_lane(self, lane: str) -> None:
        """The variable-length lanes have a segment format of their own:
        a writer takes either them or the other write_* lanes, and only
        one of the two variable-length lanes."""
        varlen = lane in ("write_varlen", "write_device_varlen")
        used = {
            "write_batch": bool(self._key_batches),
            "write_device_batch": bool(self._gpu_batches),
            "write_device_records": bool(self._gpu_records),
            "write_records": self._byte_records is not None,
            "write_varlen": bool(self._varlen_batches),
            "write_device_varlen": bool(self._gpu_varlen),
        }
        for other, on in used.items():
            if on and other != lane and (
                    varlen or other in ("write_varlen",
                                        "write_device_varlen")):
                raise ValueError(f"{lane} cannot be mixed with {other} in "
                                 "one writer")

    def write_varlen(self, keys, offsets, data) -> None:
        """CPU lane for rows of a u64 key and a payload of any length, in
        the CSR / Arrow binary layout: ``keys`` numpy u64[n], ``offsets``
        int64[n + 1] with ``offsets[0] == 0``, row r is
        ``data[offsets[r]:offsets[r + 1]]`` of the uint8 array ``data``.
        Several batches concatenate. Offsets that are not such a scan
        raise ValueError here. Read back with ``read_varlen``."""
        from .varlen import check_offsets
        self._check_lane("write_varlen")
        keys = np.ascontiguousarray(keys).astype(np.uint64, copy=False) \
            .reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        check_offsets(offsets, len(keys), len(data))
        self._varlen_batches.append((keys, offsets, data))

    def write_device_varlen(self, keys, offsets, data) -> None:
        """GPU lane of ``write_varlen``: ``keys`` int64[n] (u64 bits),
        ``offsets`` int64[n + 1] and ``data`` uint8 are CUDA tensors.
        Nothing is read here and the call does not synchronise; the rows
        are partitioned and laid out in HBM pool blocks at stop()
        (ops/csrc/varlen.hip), and the offsets are checked there:
        ``offsets[0] == 0``, non-decreasing, ``offsets[-1] <=
        data.numel()`` — a violation raises ValueError from stop() before
        anything is published.

        Limits: a partitioner with ``gpu_params()`` that is not a search of
        split points, at most 4096 partitions, no map-side combine."""
        import torch
        self._check_lane("write_device_varlen")
        for t, name, dt in ((keys, "keys", torch.int64),
                            (offsets, "offsets", torch.int64),
                            (data, "data", torch.uint8)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt \
                    or t.dim() != 1 or not t.is_cuda:
                raise ValueError(f"{name} must be a 1-D {dt} CUDA tensor")
        if offsets.numel() != keys.numel() + 1:
            raise ValueError(f"offsets has {offsets.numel()} entries for "
                             f"{keys.numel()} keys, expected "
                             f"{keys.numel() + 1}")
        self._gpu_varlen.append((keys.contiguous(), offsets.contiguous(),
                                 data.contiguous()))

    # -- commit ---------------------------------------------------------

    def stop(self, success: bool, partitioner=None, combiner=None,
             combine_key_bits: int = 64) -> None:
        """Partition, lay out and publish this map task's output.

        ``combiner`` (one of ShuffleReader.AGGREGATORS) turns on the
        map-side combine of (u64 key, u64 value) rows — what Spark's
        sort-shuffle writer does for the reference when
        ``dep.mapSideCombine`` is set: the task's rows are sorted by key,
        collapsed to ONE row per distinct key, and only those are
        partitioned and shipped. After "count" the shipped value is this
        map's row count for the key. The reduce side must then merge:
        ``read_aos(aggregator=combiner, map_side_combined=True)``.
        ``metrics.records_written`` / ``bytes_written`` count the combined
        rows; ``metrics.extra["records_combined_in"]`` the input rows.

        ``combine_key_bits`` < 64 sorts by the low key bits only, which
        saves radix passes for callers with a bounded key space. Keys that
        differ above those bits then fragment each other's runs and the
        combine is partial: more rows are shipped, but the result is still
        correct because the reduce side merges.

        Supported on the 16-byte lanes (write_device_batch, and write_batch
        with 8-byte values); ``combiner=None`` is the plain path.
        """
        if self._stopped:
            return
        if combiner is not None:
            self._check_combiner(combiner, combine_key_bits)
        if success and self._gpu_varlen:
            self._check_gpu_varlen(partitioner)
        self._stopped = True
        if not success:
            return
        t0 = time.perf_counter_ns()
        if self._gpu_varlen:
            self._commit_gpu_varlen(partitioner)
        elif self._varlen_batches:
            self._commit_varlen(partitioner)
        elif self._gpu_records:
            self._commit_gpu_records(partitioner)
        elif self._gpu_batches:
            self._commit_gpu(partitioner, combiner, combine_key_bits)
        else:
            if self._byte_records is not None:
                segments = [b"".join(recs) for recs in self._byte_records]
            else:
                segments = self._partition_fixed(partitioner, combiner,
                                                 combine_key_bits)
            self._commit_segments(segments)
        self.metrics.write_ns += time.perf_counter_ns() - t0
        lm = getattr(self.manager, "lifetime_metrics", None)
        if lm is not None:
            lm.merge(self.metrics)

    def _check_combiner(self, combiner, combine_key_bits) -> None:
        """Reject what map-side combine does not cover, before any state
        changes (stop() can then be called again without a combiner)."""
        from .aggregate import check_aggregator
        check_aggregator(combiner, "combiner")
        if not 1 <= combine_key_bits <= 64:
            raise ValueError("combine_key_bits must be in [1, 64]")
        if self._gpu_records:
            raise ValueError("map-side combine does not cover wide records "
                             "(write_device_records)")
        if self._byte_records is not None:
            raise ValueError("map-side combine does not cover the pickled "
                             "lane (write_records)")
        if self._varlen_batches or self._gpu_varlen:
            raise ValueError("map-side combine does not cover "
                             "variable-length rows (write_varlen, "
                             "write_device_varlen)")
        for _k, v in self._gpu_batches:
            if v is None:
                raise ValueError("map-side combine needs values; a "
                                 "value-less batch was written")
        for v in self._value_batches:
            if v is None:
                raise ValueError("map-side combine needs values; a "
                                 "value-less batch was written")
            if v.ndim != 2 or v.shape[1] != 8:
                raise ValueError("map-side combine needs 8-byte values, got "
                                 f"shape {v.shape}")

    def _partition_fixed(self, partitioner, combiner=None,
                         combine_key_bits: int = 64) -> List[bytes]:
        R = self.handle.num_partitions
        if not self._key_batches:
            return [b""] * R
        keys = (self._key_batches[0] if len(self._key_batches) == 1
                else np.concatenate(self._key_batches))
        vals = None
        if self._value_batches and self._value_batches[0] is not None:
            vals = (self._value_batches[0] if len(self._value_batches) == 1
                    else np.concatenate(self._value_batches))
        if combiner is not None:
            # numpy mirror of the GPU lane: stable sort by the low key
            # bits, then one row per run of equal (full) keys
            from .aggregate import reduce_sorted_np
            self.metrics.extra["records_combined_in"] = \
                self.metrics.extra.get("records_combined_in", 0) + len(keys)
            v64 = np.ascontiguousarray(vals).view(np.uint64).reshape(-1)
            skey = keys if combine_key_bits >= 64 else \
                keys & np.uint64((1 << combine_key_bits) - 1)
            order = np.argsort(skey, kind="stable")
            keys, red = reduce_sorted_np(keys[order], v64[order], combiner)
            if red.dtype == np.float64:
                red = red.view(np.uint64)
            vals = np.ascontiguousarray(red.astype(np.uint64, copy=False)) \
                .view(np.uint8).reshape(-1, 8)
        pids = partitioner.partition_ids(keys)
        order = np.argsort(pids, kind="stable")
        keys_sorted = keys[order]
        vals_sorted = vals[order] if vals is not None else None
        counts = np.bincount(pids, minlength=R)
        ends = np.cumsum(counts)
        starts = ends - counts
        self.metrics.records_written += len(keys)
        return [pack_partition_segment(
                    keys_sorted[starts[p]:ends[p]],
                    vals_sorted[starts[p]:ends[p]] if vals_sorted is not None else None)
                for p in range(R)]

    def _gpu_part_params(self, partitioner):
        """(func, shift, nparts, nbits_eff) for the kernel-side partition
        function (partitioner.gpu_params()): pow2 R via bit extraction,
        arbitrary R via mulhi-range / hash-mod / a search of the
        partitioner's split points (func 4, record lane only). One kernel
        pass covers nbits <= 12; larger R runs the two-level pid radix
        (_group_pairs_2level), capped at 2^24."""
        R = self.handle.num_partitions
        nbits = max((R - 1).bit_length(), 1)
        if nbits > 24:
            raise ValueError(
                f"GPU partitioner supports R <= 2^24, got {R}; "
                "use the CPU write path for larger partition counts")
        params = None
        if hasattr(partitioner, "gpu_params"):
            params = partitioner.gpu_params()
        elif hasattr(partitioner, "gpu_shift"):
            params = (0, partitioner.gpu_shift, 0)
        if params is None:
            raise ValueError(
                f"partitioner {partitioner!r} has no GPU dispatch (no "
                "gpu_params(), or it returned None) — use the CPU write "
                "path")
        func, shift, nparts = params
        return func, shift, nparts, min(max(nbits, 4), 12)

    def _commit_gpu(self, partitioner, combiner=None,
                    combine_key_bits: int = 64) -> None:
        """Map-side GPU write: one radix pass whose scatter writes each
        partition's [keys|vals] segment STRAIGHT into its final position in
        HBM pool blocks (the north-star replacement for the reference's
        CPU writer + mmap + register, RdmaMappedFile.java:113-189)."""
        import torch
        from .ops import load as ops_load
        from .ops.radix import digit_counts
        if self.manager.gpu is None:
            raise RuntimeError("GPU writer requires the GPU data plane")
        hs = ops_load()
        R = self.handle.num_partitions
        batches = self._gpu_batches
        keys = (batches[0][0] if len(batches) == 1
                else torch.cat([b[0] for b in batches]))
        vals = (batches[0][1] if len(batches) == 1 or batches[0][1] is None
                else torch.cat([b[1] for b in batches]))
        if combiner is not None:
            # map-side combine: sort this task's rows by key, collapse
            # each run to one row (ops/csrc/reduce.hip), carry on with
            # the combined rows
            from .ops.radix import reduce_by_key_aos, sort_pairs_aos
            self.metrics.extra["records_combined_in"] = \
                self.metrics.extra.get("records_combined_in", 0) \
                + keys.numel()
            pr = torch.empty(2 * keys.numel(), dtype=torch.int64,
                             device=keys.device)
            pr[0::2] = keys
            pr[1::2] = vals
            # whole 8-bit digits: extra sorted bits only combine more
            pr = sort_pairs_aos(pr, 0, min(-(-combine_key_bits // 8) * 8, 64))
            keys, vals = reduce_by_key_aos(pr, combiner)
            if vals.dtype != torch.int64:
                vals = vals.view(torch.int64)
        func, shift, nparts, nbits_eff = self._gpu_part_params(partitioner)
        if (R - 1).bit_length() > 12 or func == PART_BOUNDS:
            # > 4096 partitions: route through the wide-record two-level
            # pid radix (records = the interleaved 16-B AoS pairs, or the
            # bare keys when value-less). Split-point partitioners take
            # the record lane at every R: the direct scatter below derives
            # its digit from the key twice (hist, scatter) and has no
            # place to keep a searched partition id.
            if vals is None:
                recs = keys.contiguous().view(torch.uint8).reshape(-1)
                self._record_shape = (8, 8)
            else:
                pr = torch.empty(2 * keys.numel(), dtype=torch.int64,
                                 device=keys.device)
                pr[0::2] = keys
                pr[1::2] = vals
                recs = pr.view(torch.uint8).reshape(-1)
                self._record_shape = (16, 8)
            self._gpu_records = [recs]
            return self._commit_gpu_records(partitioner)
        has_val = vals is not None
        n = keys.numel()
        if n == 0:
            self._commit_empty()
            return
        dev = keys.device
        hist, totals = digit_counts(keys.data_ptr(), n, shift, nbits_eff, dev,
                                    func, 1, nparts)
        counts = totals.cpu().numpy().astype(np.int64)[:R]  # syncs the stream
        layout = _GpuLayout(self, counts * (16 if has_val else HEADER_W),
                            1 << nbits_eff, dev)
        # AoS segment: record r's key at +r*16, value at +r*16+8
        kd = torch.from_numpy(layout.dst).to(dev)
        vd = (torch.from_numpy(np.where(layout.dst != 0, layout.dst + 8, 0))
              .to(dev) if has_val else kd)
        hs.radix_scatter(keys.data_ptr(),
                         vals.data_ptr() if has_val else 0,
                         n, shift, nbits_eff, hist.data_ptr(),
                         kd.data_ptr(), vd.data_ptr(),
                         torch.cuda.current_stream().cuda_stream, func,
                         1 if has_val else 0, 1, nparts)
        layout.finish(n)

    def _group_pairs_2level(self, recs, n, W, key_bytes, R,
                            func, shift, nparts, bounds=None):
        """> 4096 partitions: the single radix pass is capped at 2^12 LDS
        digits, so the PARTITION ID itself is radixed in two levels —
        extract (pid, aux) pairs, scatter by pid>>12 (coarse), then per
        coarse bucket by pid&4095 (fine). Returns (full R counts, grouped
        pairs, pid mask): pid is pair.x, so the gather recomputes it as
        plain bits under that mask (func 0, shift 0)."""
        import torch
        from .ops.radix import digit_counts, extract_pairs, scatter_pairs
        dev = recs.device
        mask_full = (1 << (R - 1).bit_length()) - 1   # R <= 2^24
        G = (R + 4095) >> 12
        nbits_c = max((G - 1).bit_length(), 4)
        pairs = extract_pairs(recs, W, key_bytes, bounds=bounds,
                              pid=(func, shift, mask_full, nparts))
        # coarse: group by pid >> 12
        hist, totals_c = digit_counts(pairs.data_ptr(), n, 12, nbits_c, dev,
                                      0, 2)
        counts_c = totals_c.cpu().numpy().astype(np.int64)[:G]   # sync
        starts_c = np.cumsum(counts_c) - counts_c
        pairs_c = torch.empty_like(pairs)
        bases_c = torch.from_numpy(
            np.pad(starts_c, (0, (1 << nbits_c) - G))).to(dev)
        scatter_pairs(pairs, n, 12, nbits_c, hist,
                      pairs_c.data_ptr() + bases_c * 16)
        # fine: per coarse bucket, group its subrange by pid & 4095.
        # All fine hists run first (stream-ordered, per-bucket totals
        # persist), ONE sync, then all fine scatters.
        totals_f = torch.zeros(G * 4096, dtype=torch.int32, device=dev)
        fine = []
        for b in range(G):
            cnt = int(counts_c[b])
            if cnt == 0:
                continue
            sub = pairs_c[2 * starts_c[b]:2 * (starts_c[b] + cnt)]
            span = slice(b * 4096, (b + 1) * 4096)
            bh, _ = digit_counts(sub.data_ptr(), cnt, 0, 12, dev, 0, 2,
                                 totals=totals_f[span])
            fine.append((bh, sub, cnt, span))   # bh lives on to the scatter
        counts_full = totals_f.cpu().numpy().astype(np.int64)[:R]   # sync
        # pids b*4096+j with j beyond R's tail never occur; length R slice
        starts_full = np.cumsum(counts_full) - counts_full
        pairs_f = pairs   # reuse: original extraction no longer needed
        base_addr = torch.from_numpy(np.pad(
            pairs_f.data_ptr() + starts_full * 16,
            (0, G * 4096 - R))).to(dev)
        for bh, sub, cnt, span in fine:
            scatter_pairs(sub, cnt, 0, 12, bh, base_addr[span])
        return counts_full, pairs_f, mask_full

    def _commit_gpu_records(self, partitioner) -> None:
        """Wide-record map-side GPU write. Every record moves once, from
        where the task left it straight to its final HBM position
        (ops/csrc/kernels.hip 'wide-record machinery'); only 16-byte pairs
        run the radix machinery before that. Up to 256 partitions (a digit
        of at most 8 bits): the pairs carry the partition id, whether bits,
        range, hash or split points produced it; their ids are counted for
        the block layout, and ONE fused pass ranks the pairs, finds every
        tile's place in its partitions and writes the records there, in
        input order (ops/radix.py count_record_digits / group_records).
        Digits of 9 to 12 bits group the pairs through the per-tile
        histogram matrix and then gather the records; more than 4096
        partitions group the pairs in two levels first. Replaces the
        reference's CPU writer + mmap + register for arbitrary-width
        records (RdmaMappedFile.java:113-189)."""
        import torch
        from .ops.radix import (count_record_digits, gather_grouped,
                                group_records)
        if self.manager.gpu is None:
            raise RuntimeError("GPU writer requires the GPU data plane")
        R = self.handle.num_partitions
        func, shift, nparts, nbits_eff = self._gpu_part_params(partitioner)
        W, key_bytes = self._record_shape
        batches = self._gpu_records
        recs = (batches[0] if len(batches) == 1 else torch.cat(batches))
        n = recs.numel() // W
        if n == 0:
            self._commit_empty()
            return
        dev = recs.device
        # split-point partitioner: the extract searches the bounds and
        # leaves the partition id in pair.x
        bounds = (partitioner.gpu_bounds(dev) if func == PART_BOUNDS
                  else None)
        if bounds is not None and bounds.numel() != R - 1:
            # an id >= R would have no destination block
            raise ValueError(
                f"partitioner has {bounds.numel()} split points, the "
                f"shuffle was registered with {R} partitions")
        if (R - 1).bit_length() > 12:
            # the pairs are grouped while the counts are discovered
            counts, grouped, mask = self._group_pairs_2level(
                recs, n, W, key_bytes, R, func, shift, nparts, bounds)
            layout = _GpuLayout(self, counts * W, R, dev)
            gather_grouped(recs, grouped, n, W, counts, layout.dst, 0, mask)
        else:
            digits = count_record_digits(recs, W, key_bytes, shift,
                                         nbits_eff, func, nparts, bounds)
            counts = digits.counts                          # synced
            if counts[R:].any():
                # such a record would have no destination block
                raise ValueError("partitioner produced an id >= "
                                 f"{R} on the GPU")
            layout = _GpuLayout(self, counts[:R] * W, 1 << nbits_eff, dev)
            group_records(recs, W, digits, layout.dst)
        layout.finish(n)

    # -- variable-length rows -------------------------------------------

    VARLEN_MAX_PARTITIONS = 4096

    def _commit_varlen(self, partitioner) -> None:
        """CPU lane: the numpy mirror of _commit_gpu_varlen."""
        from .varlen import concat_rows, partition_varlen_np
        keys, offsets, data = concat_rows(self._varlen_batches)
        pids = partitioner.partition_ids(keys)
        self.metrics.records_written += len(keys)
        self._commit_segments(partition_varlen_np(
            keys, offsets, data, pids, self.handle.num_partitions))

    def _check_gpu_varlen(self, partitioner) -> None:
        """Reject what the GPU variable-length lane does not cover, before
        any state changes."""
        R = self.handle.num_partitions
        limit = self.VARLEN_MAX_PARTITIONS
        if R > limit:
            raise ValueError(
                f"write_device_varlen supports R <= {limit} partitions, got "
                f"{R}; use write_varlen (the CPU lane) beyond that")
        func = self._gpu_part_params(partitioner)[0]
        if func == PART_BOUNDS:
            raise ValueError(
                "write_device_varlen does not cover split-point partitioners "
                "(a search of gpu_bounds()); it takes partitioners whose "
                f"gpu_params() is a closed form, at R <= {limit}")

    def _commit_gpu_varlen(self, partitioner) -> None:
        """Map-side GPU write of variable-length rows. (key, row id) pairs
        run the 16-byte pair machinery and are grouped by partition; the
        lengths follow in grouped order and their scan places every
        payload; ONE byte-balanced copy (ops/csrc/varlen.hip) then writes
        every partition's segment — header, index, heap, padding — to its
        final position in the HBM pool blocks. The header plus index slab of
        a partition is built with torch on the device and copied as one
        long row; the padding is a row of zeros."""
        import torch
        from .ops.radix import digit_counts, scatter_pairs
        from .ops.varlen import exclusive_scan, varlen_copy
        from .varlen import ALIGN, HEADER_BYTES, INDEX_ENTRY_BYTES
        if self.manager.gpu is None:
            raise RuntimeError("GPU writer requires the GPU data plane")
        R = self.handle.num_partitions
        func, shift, nparts, nbits_eff = self._gpu_part_params(partitioner)
        nd = 1 << nbits_eff
        batches = self._gpu_varlen
        n = sum(b[0].numel() for b in batches)
        if n == 0:
            self._commit_empty()
            return
        dev = batches[0][0].device
        # rows of all batches: length and source address; the offsets check
        # stays on the device until the counts come back
        bad = torch.zeros((), dtype=torch.bool, device=dev)
        lens, addrs = [], []
        for _k, off, data in batches:
            d = off[1:] - off[:-1]
            bad = bad | (off[0] != 0) | (off[-1] > data.numel())
            if d.numel():
                bad = bad | (d.min() < 0)
            lens.append(d)
            addrs.append(off[:-1] + data.data_ptr())
        lens = lens[0] if len(lens) == 1 else torch.cat(lens)
        addrs = addrs[0] if len(addrs) == 1 else torch.cat(addrs)
        pr = torch.empty(2 * n, dtype=torch.int64, device=dev)
        pr[0::2] = batches[0][0] if len(batches) == 1 \
            else torch.cat([b[0] for b in batches])
        pr[1::2] = torch.arange(n, dtype=torch.int64, device=dev)
        # group the pairs by partition id; the bases come from the device
        # scan of the digit totals, so nothing waits for the host yet
        hist, totals = digit_counts(pr.data_ptr(), n, shift, nbits_eff, dev,
                                    func, 2, nparts)
        cnt = totals.to(torch.int64)
        ends = torch.cumsum(cnt, 0)
        starts = ends - cnt
        grouped = torch.empty_like(pr)
        scatter_pairs(pr, n, shift, nbits_eff, hist,
                      grouped.data_ptr() + starts * 16, func, nparts)
        rid = grouped[1::2]
        glen = lens[rid]
        gcum = exclusive_scan(glen)
        heap = gcum[ends] - gcum[starts]
        # THE host sync: per-partition rows, payload bytes, offsets verdict
        host = torch.cat([cnt, heap, bad.to(torch.int64).reshape(1)]) \
            .cpu().numpy()
        if host[-1]:
            raise ValueError(
                "write_device_varlen: offsets must start at 0, be "
                "non-decreasing and end inside data")
        counts, heaps = host[:nd], host[nd:2 * nd]
        if counts[R:].any():
            raise ValueError("partitioner produced an id >= "
                             f"{R} on the GPU")
        slab = np.where(counts > 0,
                        HEADER_BYTES + INDEX_ENTRY_BYTES * counts, 0)
        seg_bytes = -(-(slab + heaps) // ALIGN) * ALIGN
        layout = _GpuLayout(self, seg_bytes[:R], nd, dev)
        # header + index slabs of all partitions in one int64 tensor:
        # partition p's at word 2 * (starts[p] + p)
        ar_nd = torch.arange(nd, dtype=torch.int64, device=dev)
        ar_n = torch.arange(n, dtype=torch.int64, device=dev)
        pid = torch.repeat_interleave(ar_nd, cnt, output_size=n)
        idx = torch.empty(2 * (n + nd), dtype=torch.int64, device=dev)
        hp = 2 * (starts + ar_nd)
        idx[hp] = cnt
        idx[hp + 1] = heap
        rp = 2 * (ar_n + pid + 1)
        idx[rp] = grouped[0::2]
        idx[rp + 1] = gcum[1:] - gcum[starts][pid]
        # the rows of the copy, in destination order: per partition its
        # slab, its payloads, its zero padding (empty partitions: rows of
        # length 0, which own no byte)
        m = n + 2 * nd
        zeros = torch.zeros(ALIGN, dtype=torch.uint8, device=dev)
        slab_t = torch.from_numpy(slab).to(dev)
        pad_t = torch.from_numpy(seg_bytes - slab - heaps).to(dev)
        e_slab = starts + 2 * ar_nd
        e_row = ar_n + 2 * pid + 1
        e_pad = ends + 2 * ar_nd + 1
        row_len = torch.empty(m, dtype=torch.int64, device=dev)
        row_src = torch.empty(m, dtype=torch.int64, device=dev)
        row_len[e_slab] = slab_t
        row_src[e_slab] = idx.data_ptr() + 8 * hp
        row_len[e_row] = glen
        row_src[e_row] = addrs[rid]
        row_len[e_pad] = pad_t
        row_src[e_pad] = zeros.data_ptr()
        seg_first = torch.cat([e_slab, torch.tensor([m], dtype=torch.int64,
                                                    device=dev)])
        varlen_copy(exclusive_scan(row_len), row_src, seg_first,
                    torch.from_numpy(layout.dst).to(dev),
                    total=int(seg_bytes.sum()))
        layout.finish(n)

    def _commit_empty(self) -> None:
        """Zero-record map task: publish an all-empty location table."""
        mgr = self.manager
        R = self.handle.num_partitions
        table, table_addr = mgr.alloc_table(R, self.handle.shuffle_id)
        meta_key = make_key(mgr.executor_id, 1)
        for p in range(R):
            table.put(p, 0, 0, meta_key)
        mgr.keep_alive(self.handle, self.map_id, [])
        mgr.publish_map_output(self.handle, self.map_id, table_addr)

    def _commit_segments(self, segments: List[bytes]) -> None:
        """Greedy chunking at partition boundaries + table fill + publish."""
        mgr = self.manager
        write_block = mgr.conf.shuffle_write_block_size
        table, table_addr = mgr.alloc_table(self.handle.num_partitions,
                                    self.handle.shuffle_id)
        blocks = []
        meta_key = make_key(mgr.executor_id, 1)  # META_SEGMENT_ID
        for parts in group_partitions([len(seg) for seg in segments],
                                      write_block):
            total = sum(len(segments[p]) for p in parts)
            if total == 0:
                for p in parts:
                    table.put(p, 0, 0, meta_key)
                continue
            blk = mgr.pool.get(total)
            seg = mgr.data_segment(blk.segment_id)
            key = make_key(mgr.executor_id, blk.segment_id)
            off = blk.offset
            for p in parts:
                data = segments[p]
                if data:
                    seg.write(off, data)
                table.put(p, off, len(data), key)
                off += len(data)
                self.metrics.bytes_written += len(data)
            blocks.append(blk)
        mgr.keep_alive(self.handle, self.map_id, blocks)
        mgr.publish_map_output(self.handle, self.map_id, table_addr)
