"""Shuffle read path — the 3-hop one-sided fetch pipeline.

Re-design of RdmaShuffleReader.scala + RdmaShuffleFetcherIterator.scala
(the reference's hot path). Same structure:

* HOP 1: read the whole driver table once, cached per shuffle
  (RdmaShuffleManager.scala:341-376) — here a polled shm read (driver RPC
  lane across hosts).
* HOP 2: per map task, one-sided read of its MapTaskOutput entries for
  [start_partition, end_partition] (RdmaShuffleFetcherIterator.scala:
  297-311). Issued ASYNC, grouped per source executor, through the fetch
  pool — never on the constructing thread's critical path (the reference
  runs hop 2 inside table-read onComplete callbacks the same way).
* HOP 3: coalesce consecutive block locations up to shuffle_read_block_size
  (:240-263), gate on max_bytes_in_flight (:264-273) and a per-SOURCE
  request cap (:82-83 — per channel in the reference; per source executor
  here, so one hot peer's xGMI link cannot starve the others), randomize
  the pending queue to spread load across source executors (:74-79), then
  issue one-sided data reads; results surface through a blocking queue as
  they land (:340-382).

Completion model (event-driven, RdmaChannel.java:683-870 +
RdmaThread.java:45-58): GPU one-sided reads are ENQUEUED (hipMemcpyAsync
batch + recorded event = the signaled last WR) and a single completion
thread polls the in-flight events, dispatching results — in-flight depth
is set by the flow-control caps, not by a count of blocked threads. Host
segment preads and the cross-host TCP lane still run on the small thread
pool (they are genuinely blocking OS calls).
"""

from __future__ import annotations

import bisect
import os
import queue
import random
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterator, List, Optional

from .manager import ShuffleHandle, ShuffleManager
from .map_output import ENTRY_SIZE, MapTaskOutput, split_key
from .stats import TaskMetrics


@dataclass(frozen=True)
class BlockRef:
    """One shuffle block to fetch: (map_id, partition) at (key, addr, len)."""
    map_id: int
    partition: int
    key: int
    addr: int
    length: int


@dataclass
class CoalescedFetch:
    """One one-sided read covering >=1 consecutive blocks (same segment,
    contiguous addresses) — the reference's scatter-list READ collapses to
    a single contiguous read here because consecutive partitions of one map
    task are laid out back-to-back by the writer."""
    key: int
    addr: int
    length: int
    blocks: List[BlockRef]
    arena_off: int = -1          # destination offset in the fetch arena


@dataclass
class FetchResult:
    fetch: Optional[CoalescedFetch]
    data: Optional[bytes]
    error: Optional[BaseException] = None
    latency_ms: float = 0.0


_SENTINEL = FetchResult(None, None)   # wake-up after async hop-2 drains


class FetchFailedError(RuntimeError):
    """Analog of Spark's FetchFailedException — one failure fails the task
    (reference RdmaShuffleFetcherIterator.scala:167)."""


def parse_cpu_list(spec: str) -> list:
    """Parse the reference's cpuList format '0-3,8,10-11'
    (RdmaShuffleConf.scala:89) into a CPU id list for fetch-thread
    affinity (the CQ-poller placement analog, RdmaThread.java:45-47)."""
    cpus = []
    for part in (spec or "").split(","):
        part = part.strip()
        if not part:
            continue
        if "-" in part:
            a, b = part.split("-")
            cpus.extend(range(int(a), int(b) + 1))
        else:
            cpus.append(int(part))
    return cpus


def coalesce_blocks(blocks: List[BlockRef], max_bytes: int,
                    max_blocks: int = 1 << 30) -> List[CoalescedFetch]:
    """Group blocks into minimal one-sided reads.

    Blocks merge while they are in the same segment AND contiguous AND the
    running size stays under max_bytes (reference :240-263; a block larger
    than max_bytes still fetches as one read). Zero-length blocks are
    dropped.
    """
    out: List[CoalescedFetch] = []
    cur: Optional[CoalescedFetch] = None
    for b in blocks:
        if b.length == 0:
            continue
        if (cur is not None and b.key == cur.key
                and b.addr == cur.addr + cur.length
                and cur.length + b.length <= max_bytes
                and len(cur.blocks) < max_blocks):
            cur.blocks.append(b)
            cur.length += b.length
        else:
            cur = CoalescedFetch(b.key, b.addr, b.length, [b])
            out.append(cur)
    return out


class DeviceView:
    """A zero-copy window on device memory that is not a torch tensor: a
    run of records a reader left IN PLACE in one of the shuffle's HBM
    blocks (raw slab memory). ``ptr`` / ``data_ptr()`` is its device
    address, ``arena_off`` the offset it would have had in the fetch arena
    (pair indices count from there). Slicing gives a narrower view.

    Valid until the shuffle that owns the block is unregistered."""

    __slots__ = ("ptr", "length", "arena_off")

    def __init__(self, ptr: int, length: int, arena_off: int):
        self.ptr, self.length, self.arena_off = ptr, length, arena_off

    def __len__(self) -> int:
        return self.length

    def numel(self) -> int:
        return self.length

    def data_ptr(self) -> int:
        return self.ptr

    def __getitem__(self, s: slice) -> "DeviceView":
        if not isinstance(s, slice):
            raise TypeError("a DeviceView is sliced, not indexed")
        a, b, step = s.indices(self.length)
        if step != 1:
            raise ValueError("a DeviceView slice is contiguous")
        return DeviceView(self.ptr + a, max(b - a, 0), self.arena_off + a)

    def __repr__(self) -> str:
        return (f"DeviceView(ptr={self.ptr:#x}, length={self.length}, "
                f"arena_off={self.arena_off})")


def build_record_segments(ranges, rec_bytes: int,
                          total_records: Optional[int] = None) -> List[tuple]:
    """The segment table of a set of record ranges.

    ``ranges``: ``(first_rec, nrec, device_ptr)`` in any order — records
    ``[first_rec, first_rec + nrec)`` of the virtual arena lie at
    ``device_ptr``, ``rec_bytes`` apart. Returns the same triples sorted by
    ``first_rec``, with neighbours that are contiguous in address merged
    and empty ranges dropped. The ranges must cover ``[0, total)`` exactly
    once (``total`` = ``total_records``, or wherever they end): a gap or an
    overlap raises ValueError — a consumer would otherwise gather records
    from the wrong place."""
    out: List[tuple] = []
    pos = 0
    for first, nrec, ptr in sorted((int(a), int(n), int(p))
                                   for a, n, p in ranges):
        if nrec < 0:
            raise ValueError(f"negative record count at record {first}")
        if nrec == 0:
            continue
        if first > pos:
            raise ValueError(f"records [{pos}, {first}) are in no segment")
        if first < pos:
            raise ValueError(f"records [{first}, {min(pos, first + nrec)}) "
                             "are in two segments")
        if out and out[-1][2] + out[-1][1] * rec_bytes == ptr:
            out[-1] = (out[-1][0], out[-1][1] + nrec, out[-1][2])
        else:
            out.append((first, nrec, ptr))
        pos = first + nrec
    if total_records is not None and pos != total_records:
        raise ValueError(f"segments end at record {pos}, expected "
                         f"{total_records}")
    return out


class FetcherIterator:
    """Async fetch pipeline with byte-budget + per-source flow control."""

    def __init__(self, manager: ShuffleManager, handle: ShuffleHandle,
                 start_partition: int, end_partition: int,
                 num_workers: int = 8, seed: Optional[int] = None,
                 arena: Optional[object] = None,
                 records: Optional[tuple] = None,
                 in_place: bool = False):
        """``records``: optional wide-record spec ``(rec_bytes, key_bytes,
        pairs)``, ``pairs`` an int64 device tensor with two elements per
        record the arena hint can hold. Event-lane fetches whose arena
        offset and length are whole records then run as the fused copy +
        pair-extract kernel: record ``arena_off // rec_bytes + i`` gets its
        (prefix, aux) pair at that index of ``pairs``. ``pair_ranges()``
        and ``pairs_written()`` say which arena ranges were served that
        way; every other fetch is a plain copy and the caller extracts.

        ``in_place=True`` (with ``records``) declares that the consumer
        takes the records through ``record_segments()`` and not through
        ``arena``. Under conf ``fusedRecordFetch=inplace`` a fetch that
        qualifies for the fused lane in ``local`` mode — the block belongs
        to this executor, a GPU key, whole records, 4-byte aligned — is
        then NOT copied: only its pairs are extracted, at the indices its
        (now purely virtual) arena offset gives, and iteration yields a
        ``DeviceView`` of the block itself instead of an arena slice.
        Every other fetch is copied into the arena as always. Once any
        range is in place ``arena`` is None — the buffer has holes — and
        ``total_bytes`` gives the extent.

        LIFETIME: in-place segments and views point into the shuffle's
        registered blocks. They are valid until ``unregister_shuffle``;
        the consumer must have synchronised the GPU work that reads them
        before it unregisters. Under ``local``/``host``/``off``, or without
        ``in_place``, nothing is left in place and ``record_segments()``
        points into the arena only."""
        self.manager = manager
        self.handle = handle
        self.start_partition = start_partition
        self.end_partition = end_partition  # inclusive
        self.metrics = TaskMetrics()
        conf = manager.conf
        self._cpus = parse_cpu_list(conf.cpu_list)
        self._max_bytes_in_flight = conf.max_bytes_in_flight
        self._read_block = conf.shuffle_read_block_size
        # per-SOURCE outstanding-read cap (reference caps per channel:
        # RdmaShuffleFetcherIterator.scala:82-83)
        self._per_source_limit = conf.resolved_read_requests_limit()
        self._results: "queue.Queue[FetchResult]" = queue.Queue()
        self._pending: List[CoalescedFetch] = []
        self._lock = threading.Lock()
        self._bytes_in_flight = 0
        self._reqs_by_source: dict = {}
        self._outstanding = 0     # fetches created, not yet surfaced
        self._hop2_pending = 1    # +1 sentinel for the submit phase itself
        self._pool = ThreadPoolExecutor(max_workers=num_workers,
                                        thread_name_prefix="sparkrdma-fetch",
                                        initializer=self._pin_worker)
        self._rng = random.Random(seed)
        self._failed: Optional[BaseException] = None
        self._done = threading.Event()
        # fetch arena: one device buffer all GPU one-sided reads land in at
        # pre-assigned offsets (bump-allocated as hop-2 results arrive)
        self._arena_buf = arena            # caller-provided hint (optional)
        self._arena_used = 0
        self._deferred: List[CoalescedFetch] = []  # awaiting arena alloc
        self._arena_view = None            # exact-length view, set when known
        self.total_bytes = 0               # arena extent, set with the view
        self.arena_complete = False
        self._inflight_gpu: dict = {}      # event id -> (fetch, t0)
        self._blocking_arena_inflight = 0  # pool fetches writing the arena
        self._paused = False               # arena-growth issue gate
        self._completion_thread: Optional[threading.Thread] = None
        # fused record lane (conf.fused_record_fetch); off once the arena
        # is allocated late or grows — callers re-extract such arenas whole
        self._records = records
        self._fuse_mode = (getattr(conf, "fused_record_fetch", "local")
                           if records is not None and arena is not None
                           else "off")
        self._pair_starts: List[int] = []  # sorted arena offsets ...
        self._pair_ends: dict = {}         # ... -> end of the fused range
        # ranges left in place: arena offset -> (device pointer, length)
        self._in_place = bool(in_place) and records is not None
        self._inplace_src: dict = {}
        self._pool.submit(self._start_async)

    # ------------------------------------------------------------------

    def _pin_worker(self) -> None:
        """Spread fetch workers over conf.cpuList (poller affinity parity,
        RdmaNode.java:222-279). No-op when the list is empty."""
        if self._cpus:
            try:
                os.sched_setaffinity(0, set(self._cpus))
            except OSError:
                pass

    # ------------------------------ hop 1 + 2 (async) ------------------

    def _start_async(self) -> None:
        """Runs on the pool: hop 1, then one hop-2 task per source
        executor. The constructor returns immediately; the consumer blocks
        on the results queue until data lands."""
        try:
            mgr = self.manager
            entries = mgr.get_map_task_output_table(self.handle)  # HOP 1
            groups: dict = {}   # owner exec -> [(map_id, table_addr, table_key)]
            for map_id, (table_addr, table_key) in enumerate(entries):
                owner = split_key(table_key)[0]
                groups.setdefault(owner, []).append(
                    (map_id, table_addr, table_key))
            with self._lock:
                self._hop2_pending += len(groups)
            for owner, maps in groups.items():
                self._pool.submit(self._hop2_group, owner, maps)
        except BaseException as e:
            self._results.put(FetchResult(None, None, error=e))
        finally:
            self._hop2_done()

    def _hop2_group(self, owner: int, maps: list) -> None:
        """HOP 2 for one source executor: read each of its map tasks'
        location entries (one-sided pread same-host, TCP lane across
        hosts — ADVICE r01), build + coalesce blocks, pre-resolve the
        slabs they point into, then enqueue the fetches."""
        mgr = self.manager
        span = self.end_partition - self.start_partition + 1
        try:
            blocks: List[BlockRef] = []
            remote_host = mgr.is_remote_host(owner)
            for map_id, table_addr, table_key in maps:
                addr = table_addr + self.start_partition * ENTRY_SIZE
                raw = (mgr.tcp_read(owner, table_key, addr, span * ENTRY_SIZE)
                       if remote_host
                       else mgr.remote_read(table_key, addr, span * ENTRY_SIZE))
                for i, loc in enumerate(MapTaskOutput.parse_locations(raw)):
                    blocks.append(BlockRef(map_id, self.start_partition + i,
                                           loc.key, loc.addr, loc.length))
            fetches = coalesce_blocks(blocks, self._read_block)
            # pre-resolve slab bases OFF the issue path (first IPC open of
            # a peer slab costs ms; pump()'s issue is then pure enqueue)
            if mgr.gpu is not None and not remote_host:
                from .gpu_plane import is_gpu_key
                for key in {f.key for f in fetches if is_gpu_key(f.key)}:
                    mgr.gpu.resolve(key)
            self._ingest(fetches)
        except BaseException as e:
            self._results.put(FetchResult(None, None, error=e))
        finally:
            self._hop2_done()

    def _hop2_done(self) -> None:
        with self._lock:
            self._hop2_pending -= 1
            finished = self._hop2_pending == 0
        if finished:
            self._finalize_arena()
            self._results.put(_SENTINEL)
        self._pump()

    def _ingest(self, fetches: List[CoalescedFetch]) -> None:
        """Register new fetches: assign arena destinations, randomize, add
        to the pending queue (reference randomized queue :74-79)."""
        use_arena = self.manager.gpu is not None
        with self._lock:
            if use_arena:
                for f in fetches:
                    if (self._arena_buf is not None
                            and self._arena_used + f.length
                            <= self._arena_buf.numel()):
                        f.arena_off = self._arena_used
                        self._arena_used += f.length
                    else:
                        # no hint (or hint exhausted): defer until all
                        # hop-2 results are in, then allocate exactly
                        self._deferred.append(f)
            self._rng.shuffle(fetches)
            self._pending.extend(f for f in fetches
                                 if not (use_arena and f.arena_off < 0))
            self._outstanding += len(fetches)

    def _finalize_arena(self) -> None:
        """All hop-2 results are in: place any deferred fetches (no-hint
        mode allocates the exact total now) and expose the arena view."""
        with self._lock:
            deferred, self._deferred = self._deferred, []
        if deferred:
            import torch
            self._fuse_mode = "off"
            total = sum(f.length for f in deferred)
            dev = f"cuda:{self.manager.gpu.device}"
            if self._arena_buf is None and self._arena_used == 0:
                self._arena_buf = torch.empty(total, dtype=torch.uint8,
                                              device=dev)
            else:
                # hint exhausted mid-stream: pause issuing, drain landed
                # writes, grow into a fresh buffer, copy the prefix
                with self._lock:
                    self._paused = True
                old, used = self._arena_buf, self._arena_used
                new = torch.empty(used + total, dtype=torch.uint8, device=dev)
                self._drain_inflight()
                if used:
                    new[:used] = old[:used]
                    torch.cuda.synchronize()
                self._arena_buf = new
                with self._lock:
                    self._paused = False
            with self._lock:
                for f in deferred:
                    f.arena_off = self._arena_used
                    self._arena_used += f.length
                self._pending.extend(deferred)
        if self.manager.gpu is not None and self._arena_buf is not None:
            self._arena_view = self._arena_buf[:self._arena_used]
        self.total_bytes = self._arena_used
        self.arena_complete = True

    def _drain_inflight(self) -> None:
        """Wait for every in-progress arena write to land (arena
        re-allocation barrier; rare — only when a caller's arena hint was
        undersized)."""
        while True:
            with self._lock:
                evs = list(self._inflight_gpu.keys())
                blocking = self._blocking_arena_inflight
            if not evs and blocking == 0:
                return
            for ev in evs:
                self.manager.gpu.wait_event(ev)
            time.sleep(0.0002)

    # ------------------------------ hop 3 -------------------------------

    def _pump(self) -> None:
        """Issue pending fetches while under the byte budget (reference
        :264-273, re-pumped from next() :365-374) and each source's
        outstanding-request cap (:82-83)."""
        while True:
            to_issue = []
            with self._lock:
                if self._failed is not None or self._paused:
                    return
                i = len(self._pending) - 1
                while i >= 0:
                    f = self._pending[i]
                    if (self._bytes_in_flight > 0
                            and self._bytes_in_flight + f.length
                            > self._max_bytes_in_flight):
                        break   # global byte budget: stop issuing
                    src = split_key(f.key)[0]
                    if (self._reqs_by_source.get(src, 0)
                            >= self._per_source_limit):
                        i -= 1   # this source saturated; try others
                        continue
                    self._pending.pop(i)
                    self._bytes_in_flight += f.length
                    self._reqs_by_source[src] = \
                        self._reqs_by_source.get(src, 0) + 1
                    to_issue.append(f)
                    i -= 1
            if not to_issue:
                return
            for f in to_issue:
                self._issue(f)

    def _issue(self, f: CoalescedFetch) -> None:
        from .gpu_plane import is_gpu_key
        mgr = self.manager
        owner = split_key(f.key)[0]
        if (f.arena_off >= 0 and is_gpu_key(f.key)
                and not mgr.is_remote_host(owner)):
            # event-driven lane: enqueue the xGMI copy; the completion
            # thread polls the event (no blocked thread per fetch)
            try:
                dst = self._arena_buf.data_ptr() + f.arena_off
                if self._leave_in_place(f, owner):
                    W, key_bytes, pairs = self._records
                    idx_base = f.arena_off // W
                    ev, src = mgr.gpu.issue_extract_records(
                        f.key, f.addr, f.length, W, key_bytes,
                        pairs.data_ptr() + 16 * idx_base, idx_base)
                    with self._lock:
                        bisect.insort(self._pair_starts, f.arena_off)
                        self._pair_ends[f.arena_off] = f.arena_off + f.length
                        self._inplace_src[f.arena_off] = (src, f.length)
                elif self._fused(f, owner):
                    W, key_bytes, pairs = self._records
                    idx_base = f.arena_off // W
                    ev = mgr.gpu.issue_read_records_into(
                        f.key, f.addr, f.length, dst, W, key_bytes,
                        pairs.data_ptr() + 16 * idx_base, idx_base)
                    with self._lock:
                        bisect.insort(self._pair_starts, f.arena_off)
                        self._pair_ends[f.arena_off] = f.arena_off + f.length
                else:
                    ev = mgr.gpu.issue_read_into(f.key, f.addr, f.length, dst)
            except BaseException as e:
                self._results.put(FetchResult(f, None, error=e))
                return
            with self._lock:
                self._inflight_gpu[ev] = (f, time.perf_counter())
            self._ensure_completion_thread()
        else:
            if f.arena_off >= 0:
                with self._lock:
                    self._blocking_arena_inflight += 1
            self._pool.submit(self._do_fetch_blocking, f)

    def _fused(self, f: CoalescedFetch, owner: int) -> bool:
        """Does this event-lane fetch take the fused record kernel?"""
        mode = self._fuse_mode
        if mode == "off" or (mode in ("local", "inplace")
                             and owner != self.manager.executor_id):
            return False
        W, _key_bytes, pairs = self._records
        return (f.arena_off % W == 0 and f.length % W == 0
                and f.addr % 4 == 0
                and self._arena_buf.data_ptr() % 4 == 0
                and pairs.data_ptr() % 16 == 0
                and 2 * ((f.arena_off + f.length) // W) <= pairs.numel())

    def _leave_in_place(self, f: CoalescedFetch, owner: int) -> bool:
        """Is this event-lane fetch served where it lies? Exactly the
        fetches the fused lane takes in ``local`` mode, for a reader that
        asked for it under conf ``inplace``."""
        return (self._in_place and self._fuse_mode == "inplace"
                and owner == self.manager.executor_id
                and self._fused(f, owner))

    @property
    def arena(self):
        """The fetched bytes as one device tensor — None until the extent
        is known, and None for good once any range was left in place (the
        buffer then has holes: use ``record_segments()``)."""
        with self._lock:
            if self._inplace_src:
                return None
        return self._arena_view

    def record_segments(self) -> List[tuple]:
        """Where the records are, valid once the iterator is drained:
        ``(first_rec, nrec, device_ptr)`` triples sorted by ``first_rec``
        that cover every record of the (virtual) arena exactly once,
        neighbours contiguous in address merged. A range left in place
        points into its block, everything else into the arena buffer. See
        the class docstring for how long the pointers stay valid."""
        if self._records is None:
            raise RuntimeError("record_segments() needs a record spec")
        if not self.arena_complete:
            raise RuntimeError("record_segments() before the fetch finished")
        W = self._records[0]
        total = self.total_bytes
        if total % W:
            raise ValueError(f"{total} fetched bytes are not whole "
                             f"{W}-byte records")
        with self._lock:
            placed = sorted(self._inplace_src.items())
        base = self._arena_buf.data_ptr() if self._arena_buf is not None else 0
        ranges, pos = [], 0
        for off, (src, length) in placed + [(total, (0, 0))]:
            if off > pos:     # copied bytes between two in-place ranges
                ranges.append((pos // W, (off - pos) // W, base + pos))
            ranges.append((off // W, length // W, src))
            pos = off + length
        return build_record_segments(ranges, W, total // W)

    def pair_ranges(self) -> List[tuple]:
        """Arena ranges ``(offset, length)`` whose pairs the fused lane
        wrote (complete once the iterator is drained), by offset."""
        with self._lock:
            return [(a, self._pair_ends[a] - a) for a in self._pair_starts]

    def pairs_written(self, off: int, length: int) -> bool:
        """True if arena bytes [off, off + length) lie in one fused fetch."""
        with self._lock:
            i = bisect.bisect_right(self._pair_starts, off) - 1
            return (i >= 0 and off + length
                    <= self._pair_ends[self._pair_starts[i]])

    def _ensure_completion_thread(self) -> None:
        if self._completion_thread is None:
            t = threading.Thread(target=self._completion_loop,
                                 name="sparkrdma-completion", daemon=True)
            self._completion_thread = t
            t.start()

    def _completion_loop(self) -> None:
        """The CQ-poller analog (RdmaThread.java:45-58): poll in-flight
        copy events, dispatch results as they complete."""
        if self._cpus:
            try:
                os.sched_setaffinity(0, set(self._cpus))
            except OSError:
                pass
        gpu = self.manager.gpu
        while not self._done.is_set():
            with self._lock:
                items = list(self._inflight_gpu.items())
            if not items:
                time.sleep(0.0002)
                continue
            completed = []
            for ev, (f, t0) in items:
                try:
                    if gpu.poll_event(ev):
                        completed.append((ev, f, t0, None))
                except BaseException as e:
                    completed.append((ev, f, t0, e))
            if not completed:
                time.sleep(0.00005)
                continue
            for ev, f, t0, err in completed:
                with self._lock:
                    self._inflight_gpu.pop(ev, None)
                if err is not None:
                    self._results.put(FetchResult(f, None, error=err))
                else:
                    with self._lock:
                        placed = self._inplace_src.get(f.arena_off)
                    if placed is not None:   # never a copy: the block itself
                        data = DeviceView(placed[0], f.length, f.arena_off)
                    else:
                        data = self._arena_buf[f.arena_off:
                                               f.arena_off + f.length]
                    self._results.put(FetchResult(
                        f, data,
                        latency_ms=(time.perf_counter() - t0) * 1e3))

    def _do_fetch_blocking(self, f: CoalescedFetch) -> None:
        """Blocking lane on the thread pool: host-segment preads, the
        cross-host TCP path, and uploads of host bytes into the arena."""
        from .gpu_plane import is_gpu_key
        t0 = time.perf_counter()
        arena_buf = self._arena_buf   # capture: stable across arena growth
        try:
            owner = split_key(f.key)[0]
            if f.arena_off >= 0:
                if not self.manager.is_remote_host(owner) and is_gpu_key(f.key):
                    self.manager.gpu.read_device_into(
                        f.key, f.addr, f.length,
                        arena_buf.data_ptr() + f.arena_off)
                else:  # cross-host or host-spilled bytes: upload into place
                    import torch
                    raw = (self.manager.tcp_read(owner, f.key, f.addr, f.length)
                           if self.manager.is_remote_host(owner)
                           else self.manager.remote_read(f.key, f.addr, f.length))
                    if len(raw) != f.length:
                        raise FetchFailedError(
                            f"short read: {len(raw)}/{f.length} at key={f.key:#x}")
                    arena_buf[f.arena_off:f.arena_off + f.length] = \
                        torch.frombuffer(bytearray(raw), dtype=torch.uint8) \
                        .to(arena_buf.device)
                data = arena_buf[f.arena_off:f.arena_off + f.length]
            elif self.manager.is_remote_host(owner):
                data = self.manager.tcp_read(owner, f.key, f.addr, f.length)
            elif is_gpu_key(f.key):
                data = self.manager.remote_read_device(f.key, f.addr, f.length)
            else:
                data = self.manager.remote_read(f.key, f.addr, f.length)
            if len(data) != f.length:
                raise FetchFailedError(
                    f"short read: {len(data)}/{f.length} at key={f.key:#x}")
            self._results.put(FetchResult(
                f, data, latency_ms=(time.perf_counter() - t0) * 1e3))
        except BaseException as e:  # surfaced to consumer, fails the task
            self._results.put(FetchResult(f, None, error=e))
        finally:
            if f.arena_off >= 0:
                with self._lock:
                    self._blocking_arena_inflight -= 1

    # ------------------------------------------------------------------

    def __iter__(self) -> Iterator[tuple]:
        """Yields (BlockRef, memoryview) per block, in arrival order."""
        mgr = self.manager
        my_exec = mgr.executor_id
        try:
            while True:
                with self._lock:
                    drained = (self._outstanding == 0
                               and self._hop2_pending == 0)
                # an error of hop 1 / hop 2 is queued BEFORE its task counts
                # itself done: whatever is still queued is looked at, so a
                # failure that lost the race to this check still fails the
                # task instead of ending it as if it were empty
                if drained and self._results.empty():
                    break
                t0 = time.perf_counter_ns()
                res = self._results.get()
                self.metrics.fetch_wait_ns += time.perf_counter_ns() - t0
                if res.error is not None:
                    with self._lock:
                        self._failed = res.error
                    raise FetchFailedError(
                        "fetch failed" + (
                            f" ({len(res.fetch.blocks)} blocks at "
                            f"key={res.fetch.key:#x})" if res.fetch else "")
                        + f": {res.error!r}") from res.error
                if res.fetch is None:      # sentinel: recheck termination
                    continue
                with self._lock:
                    self._bytes_in_flight -= res.fetch.length
                    src = split_key(res.fetch.key)[0]
                    self._reqs_by_source[src] = \
                        self._reqs_by_source.get(src, 1) - 1
                    self._outstanding -= 1
                self._pump()
                owner = split_key(res.fetch.key)[0]
                remote = owner != my_exec
                if remote:
                    self.metrics.remote_bytes_read += res.fetch.length
                    self.metrics.remote_blocks_fetched += len(res.fetch.blocks)
                    if mgr.reader_stats is not None:
                        mgr.reader_stats.update(owner, res.latency_ms)
                else:
                    self.metrics.local_bytes_read += res.fetch.length
                    self.metrics.local_blocks_fetched += len(res.fetch.blocks)
                data = res.data
                view = (memoryview(data)
                        if isinstance(data, (bytes, bytearray, memoryview))
                        else data)  # device tensor: torch slicing below
                off = 0
                for b in res.fetch.blocks:
                    yield b, view[off:off + b.length]
                    off += b.length
        finally:
            self._done.set()
            self._pool.shutdown(wait=False)
            lm = getattr(mgr, "lifetime_metrics", None)
            if lm is not None:   # test fakes may omit the rollup
                lm.merge(self.metrics)


class ShuffleReader:
    """Public reader: iterate raw blocks, or consume via the GENERIC
    aggregation/ordering hookup — the role the reference's reader plays
    once (deserialize -> aggregate -> ExternalSorter ordering,
    RdmaShuffleReader.scala:61-114) instead of every workload
    re-implementing it."""

    #: named reductions for read_aos(aggregator=...)
    from .aggregate import AGGREGATORS

    def __init__(self, manager: ShuffleManager, handle: ShuffleHandle,
                 start_partition: int, end_partition: int, arena=None,
                 records=None, in_place: bool = False):
        self.manager = manager
        self.handle = handle
        self.start_partition = start_partition
        self.end_partition = end_partition
        self._fixed_records = records is not None or bool(in_place)
        self.fetcher = FetcherIterator(manager, handle,
                                       start_partition, end_partition,
                                       arena=arena, records=records,
                                       in_place=in_place)

    def __iter__(self):
        return iter(self.fetcher)

    def collect_partitions(self) -> dict:
        """partition -> list of data views (one per map task, unordered)."""
        out = {p: [] for p in range(self.start_partition, self.end_partition + 1)}
        for ref, data in self.fetcher:
            out[ref.partition].append(data)
        return out

    # ---------------- generic consumption (fixed-width AoS records) ----

    def _drain_aos_pairs(self):
        """CPU lane: fetch everything, return (keys u64, values u64)
        numpy arrays (the GPU lane drains into the fetch arena instead)."""
        from .writer import unpack_partition_segment
        import numpy as np
        ks, vs = [], []
        for _ref, data in self.fetcher:
            k, v = unpack_partition_segment(data, 8)
            ks.append(np.array(k))
            vs.append(np.ascontiguousarray(v).reshape(-1, 8)
                      .view(np.uint64).reshape(-1))
        if not ks:
            return None, None
        return np.concatenate(ks), np.concatenate(vs)

    def read_aos(self, aggregator: Optional[str] = None,
                 ordering: bool = False, end_bit: int = 64,
                 sort_tmp=None, sort_ws=None,
                 map_side_combined: bool = False):
        """Consume the whole partition range of AoS (u64 key, u64 value)
        records, applying an optional keyed reduction and/or key ordering
        ON DEVICE. Returns (keys, values):

        * aggregator=None, ordering=True  -> records sorted by key bits
          [0, end_bit) (callers whose partitions share top bits pass a
          smaller end_bit and save radix passes)
        * aggregator in AGGREGATORS -> one row per distinct key, keys
          ascending; "sum_f64" treats the value payload as float64
        * both None/False -> unordered concatenated records

        ``map_side_combined=True`` says the writers ran
        ``stop(combiner=aggregator)``: the fetched rows are partial results
        and are MERGED (the reference's combineCombinersByKey branch,
        RdmaShuffleReader.scala:83-96) — "count" merges by summing the
        per-map counts, every other aggregator merges with itself.

        On the GPU lane the keyed reduction is the reduce_by_key kernel
        (ops/csrc/reduce.hip): a fixed summation order, so "sum_f64" is
        bit-reproducible.
        """
        if aggregator is not None and aggregator not in self.AGGREGATORS:
            raise ValueError(f"unknown aggregator {aggregator!r}; "
                             f"expected one of {self.AGGREGATORS}")
        if map_side_combined:
            if aggregator is None:
                raise ValueError("map_side_combined=True needs the "
                                 "aggregator the writers combined with")
            from .aggregate import MERGE_OF
            aggregator = MERGE_OF[aggregator]
        mgr = self.manager
        if mgr.gpu is not None:
            import torch
            for _ in self.fetcher:
                pass
            arena = self.fetcher.arena
            pairs = arena.view(torch.int64)
            if pairs.numel() == 0:
                empty = torch.empty(0, dtype=torch.int64,
                                    device=f"cuda:{mgr.gpu.device}")
                return empty, empty.clone()
            if aggregator is not None or ordering:
                from .ops.radix import sort_pairs_aos
                pairs = sort_pairs_aos(pairs, 0, end_bit, tmp=sort_tmp,
                                       ws=sort_ws)
            if aggregator is None:
                return pairs[0::2], pairs[1::2]
            from .ops.radix import reduce_by_key_aos
            return reduce_by_key_aos(pairs, aggregator)
        # ---- CPU path: numpy mirror of the device semantics ----
        import numpy as np
        k, v = self._drain_aos_pairs()
        if k is None:
            return np.array([], dtype=np.uint64), np.array([], dtype=np.uint64)
        if aggregator is not None or ordering:
            mask = np.uint64((1 << end_bit) - 1) if end_bit < 64 \
                else np.uint64(2 ** 64 - 1)
            order = np.argsort(k & mask, kind="stable")
            k, v = k[order], v[order]
        if aggregator is None:
            return k, v
        uk, start = np.unique(k, return_index=True)
        if aggregator == "count":
            return uk, np.diff(np.append(start, len(k)))
        if aggregator == "sum":
            return uk, np.add.reduceat(v, start)
        if aggregator == "sum_f64":
            return uk, np.add.reduceat(v.view(np.float64), start)
        fn = np.minimum if aggregator == "min" else np.maximum
        return uk, fn.reduceat(v, start)

    def dense_sum(self, key_lo: int, span: int, dtype: str = "f64"):
        """Keyed sum into a DENSE [key_lo, key_lo+span) vector without a
        sort — the iterative-workload (PageRank) reduction: every fetched
        chunk is index-added as it arrives, overlapping with in-flight
        fetches. dtype 'f64' treats payloads as float64, 'i64' as int64."""
        mgr = self.manager
        if mgr.gpu is not None:
            import torch
            tdtype = torch.float64 if dtype == "f64" else torch.int64
            sums = torch.zeros(span, dtype=tdtype,
                               device=f"cuda:{mgr.gpu.device}")
            from .utils import as_device_i64
            for _ref, data in self.fetcher:
                t = as_device_i64(data)
                idx = t[0::2] - key_lo
                val = t[1::2].contiguous()
                sums.index_add_(0, idx, val.view(tdtype)
                                if dtype == "f64" else val)
            return sums
        import numpy as np
        from .writer import unpack_partition_segment
        ndtype = np.float64 if dtype == "f64" else np.int64
        sums = np.zeros(span, dtype=ndtype)
        for _ref, data in self.fetcher:
            k, v = unpack_partition_segment(data, 8)
            idx = (np.asarray(k) - key_lo).astype(np.int64)
            np.add.at(sums, idx, np.ascontiguousarray(v).reshape(-1, 8)
                      .view(ndtype).reshape(-1))
        return sums

    def read_records(self):
        """Pickled-record lane: yields (key, value) python objects —
        the deserialize role of RdmaShuffleReader.scala:61-77."""
        import io
        import pickle
        for _ref, data in self.fetcher:
            if not isinstance(data, (bytes, bytearray, memoryview)):
                # arena mode landed the bytes in the device arena: one
                # bulk D2H (bytes() on a CUDA tensor would sync per byte)
                data = data.cpu().numpy().tobytes()
            bio = io.BytesIO(bytes(data))
            end = len(bio.getvalue())
            while bio.tell() < end:
                yield pickle.load(bio)

    # ---------------- wide records reduced per key ----------------------

    def read_records_agg(self, record_bytes: int, columns,
                         end_bit: int = 64):
        """GROUP BY over the whole partition range of ``record_bytes``-byte
        AoS records with a u64 LE key at offset 0 — what
        ``write_device_records(recs, W, key_bytes=8)`` and
        ``write_batch(keys, values[n, W - 8])`` both write. ``columns`` is
        a sequence of ``(offset_bytes, dtype, op)``, dtype in ("i32",
        "u32", "i64", "f32", "f64"), op in ("sum", "min", "max", "count")
        (aggregate.check_columns). Returns ``(keys, [one array per
        column])``: one row per distinct key, keys ascending by bits
        [0, end_bit) (callers whose partitions share top key bits pass a
        smaller end_bit); keys are int64 holding the u64 bits, a column is
        float64 for f32 / f64 dtypes and int64 otherwise (sums wrap).

        With the GPU data plane these are device tensors and no record is
        moved: ops.radix.aggregate_records sorts (key, index) pairs and
        ops/csrc/reduce_records.hip reads each record's column bytes where
        the record lies — for a reader opened with ``records=(W, 8,
        pairs)`` through ``record_segments()``, so a block left in place
        (``in_place=True``) is neither copied nor moved. The pairs are
        re-extracted per segment, whatever the fused fetch already wrote.
        LIFETIME, as for sort_records over ``record_segments()``: the
        caller synchronises the GPU before ``unregister_shuffle``.
        Without the GPU plane the result is numpy
        (aggregate.reduce_records_np)."""
        from .aggregate import check_columns, reduce_records_np
        check_columns(columns, record_bytes)
        if record_bytes < 8:
            raise ValueError("records hold a u64 key: record_bytes >= 8")
        if not 1 <= end_bit <= 64:
            raise ValueError("end_bit must be in [1, 64]")
        spec = self.fetcher._records
        if spec is not None:
            if spec[1] != 8:
                raise ValueError(f"read_records_agg handles 8-byte keys; "
                                 f"the reader's record spec has "
                                 f"key_bytes={spec[1]}")
            if spec[0] != record_bytes:
                raise ValueError(f"record_bytes={record_bytes} disagrees "
                                 f"with the reader's record spec "
                                 f"({spec[0]} bytes)")
        elif self._fixed_records:
            raise ValueError("in_place=True needs a records= spec")
        mgr = self.manager
        if mgr.gpu is not None:
            import torch
            from .ops.radix import aggregate_records
            for _ in self.fetcher:
                pass
            if spec is not None:
                total = self.fetcher.total_bytes
                if total % record_bytes:
                    raise ValueError(f"{total} fetched bytes are not whole "
                                     f"{record_bytes}-byte records")
                with torch.cuda.device(mgr.gpu.device):
                    return aggregate_records(
                        total, record_bytes, columns, end_bit=end_bit,
                        segments=self.fetcher.record_segments())
            arena = self.fetcher.arena
            if arena is None:
                arena = torch.empty(0, dtype=torch.uint8,
                                    device=f"cuda:{mgr.gpu.device}")
            arena = arena.view(torch.uint8)
            if arena.numel() % record_bytes:
                raise ValueError(f"{arena.numel()} fetched bytes are not "
                                 f"whole {record_bytes}-byte records")
            return aggregate_records(arena, record_bytes, columns,
                                     end_bit=end_bit)
        # ---- CPU path: numpy mirror of the device semantics ----
        import numpy as np
        blocks = []
        for _ref, data in self.fetcher:
            blk = np.frombuffer(bytes(data), dtype=np.uint8)
            if len(blk) % record_bytes:
                raise ValueError(f"a fetched block of {len(blk)} bytes is "
                                 f"not whole {record_bytes}-byte records")
            blocks.append(blk)
        recs = (np.concatenate(blocks) if blocks
                else np.empty(0, np.uint8)).reshape(-1, record_bytes)
        return reduce_records_np(recs, columns, end_bit)

    # ---------------- variable-length rows (varlen.py) -----------------

    def read_varlen(self, ordering: bool = False, end_bit: int = 64):
        """Consume the whole partition range of variable-length rows
        (``write_varlen`` / ``write_device_varlen``). Returns ``(keys,
        offsets, data)`` in the CSR layout the writer took: ``keys`` has n
        entries, ``offsets`` is int64[n + 1] with ``offsets[0] == 0`` and
        row r is ``data[offsets[r]:offsets[r + 1]]`` (uint8). An empty
        range gives n = 0 and ``offsets == [0]``.

        With the GPU data plane the three are device tensors (keys int64
        holding u64 bits) and the payloads are moved by the byte-balanced
        copy of ops/csrc/varlen.hip; without it they are numpy arrays.
        ``ordering=True`` sorts the rows by key bits [0, end_bit)
        (unsigned); the order among equal keys is unspecified. Not
        available on a reader opened with ``records=`` or
        ``in_place=True``: those describe fixed-width records."""
        if self._fixed_records:
            raise ValueError("read_varlen is not available on a reader "
                             "opened with records= or in_place=True")
        if not 1 <= end_bit <= 64:
            raise ValueError("end_bit must be in [1, 64]")
        if self.manager.gpu is not None:
            return self._read_varlen_gpu(ordering, end_bit)
        import numpy as np
        from .varlen import concat_rows, take_rows, unpack_varlen_segment
        keys, offsets, data = concat_rows(
            [unpack_varlen_segment(bytes(blk)) for _ref, blk in self.fetcher])
        if ordering and len(keys):
            mask = np.uint64((1 << end_bit) - 1) if end_bit < 64 \
                else np.uint64(2 ** 64 - 1)
            order = np.argsort(keys & mask, kind="stable")
            keys = keys[order]
            offsets, data = take_rows(offsets, data, order)
        return keys, offsets, data

    def _read_varlen_gpu(self, ordering: bool, end_bit: int):
        """Drain into the arena, read every block's header with one D2H
        copy, then two byte-balanced copies: the blocks' index sections
        into one (key, end) table, and — after the optional sort of (key,
        row id) pairs — the payloads into one contiguous heap."""
        import numpy as np
        import torch
        from .ops.varlen import exclusive_scan, varlen_copy
        from .varlen import (HEADER_BYTES, INDEX_ENTRY_BYTES, segment_bytes)
        dev = torch.device("cuda", self.manager.gpu.device)
        blocks = [blk for _ref, blk in self.fetcher if len(blk)]
        for blk in blocks:
            if len(blk) % 16 or blk.data_ptr() % 16:
                raise ValueError("a fetched block is not a 16-byte aligned "
                                 "variable-length segment")

        def i64(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)) \
                .to(dev)

        S = len(blocks)
        head = (torch.cat([b[:HEADER_BYTES] for b in blocks])
                .view(torch.int64).cpu().numpy().reshape(S, 2)
                if S else np.zeros((0, 2), dtype=np.int64))   # THE sync
        nb, hb = head[:, 0], head[:, 1]
        for b, blk in enumerate(blocks):
            if nb[b] <= 0 or hb[b] < 0 \
                    or segment_bytes(int(nb[b]), int(hb[b])) != len(blk):
                raise ValueError(
                    f"block header (n={nb[b]}, H={hb[b]}) does not match "
                    f"its length {len(blk)}: not a variable-length segment")
        n, heap = int(nb.sum()), int(hb.sum())
        if n == 0:
            return (torch.empty(0, dtype=torch.int64, device=dev),
                    torch.zeros(1, dtype=torch.int64, device=dev),
                    torch.empty(0, dtype=torch.uint8, device=dev))
        ptr = np.array([blk.data_ptr() for blk in blocks], dtype=np.int64)
        first = np.cumsum(nb) - nb
        # the index sections, back to back: S rows of 16 * n_b bytes
        index = torch.empty(2 * n, dtype=torch.int64, device=dev)
        varlen_copy(i64(np.concatenate([[0], np.cumsum(nb)])
                        * INDEX_ENTRY_BYTES),
                    i64(ptr + HEADER_BYTES), i64([0, S]),
                    i64([index.data_ptr()]), total=INDEX_ENTRY_BYTES * n)
        keys, ends = index[0::2], index[1::2]
        # `end` restarts in every block: a row starts where the row before
        # it ends, a block's first row at 0
        prev = torch.zeros(n, dtype=torch.int64, device=dev)
        prev[1:] = ends[:-1]
        prev[i64(first)] = 0
        lens = ends - prev
        blk_of = torch.repeat_interleave(
            torch.arange(S, dtype=torch.int64, device=dev), i64(nb),
            output_size=n)
        src = i64(ptr + HEADER_BYTES + INDEX_ENTRY_BYTES * nb)[blk_of] + prev
        if ordering:
            from .ops.radix import sort_pairs_aos
            pr = torch.empty(2 * n, dtype=torch.int64, device=dev)
            pr[0::2] = keys
            pr[1::2] = torch.arange(n, dtype=torch.int64, device=dev)
            pr = sort_pairs_aos(pr, 0, end_bit)
            keys, order = pr[0::2], pr[1::2]
            lens, src = lens[order], src[order]
        offsets = exclusive_scan(lens)
        data = torch.empty(heap, dtype=torch.uint8, device=dev)
        varlen_copy(offsets, src.contiguous(), i64([0, n]),
                    i64([data.data_ptr()]), total=heap)
        return keys.contiguous(), offsets, data

    @property
    def metrics(self) -> TaskMetrics:
        return self.fetcher.metrics
