"""Partitioners: key -> reduce-partition id.

The reference delegates partitioning to Spark's Partitioner inside the
sort-shuffle writers (RdmaWrapperShuffleWriter.scala:83-102). The rebuild
owns it: partition-id computation is vectorized (numpy on host, HIP kernel
on GPU — ops/hipshuffle kernels use the same functions bit-for-bit).

GPU dispatch: ``gpu_params()`` returns (func, shift, nparts) selecting the
kernel-side partition function (kernels.hip ``PartFunc``):
  0 bits       (key >> shift) & (R-1)        pow2 R
  1 hash+bits  (mix(key) >> shift) & (R-1)   pow2 R >= 16
  2 range      mulhi(key, R)                 ANY R  (uniform u64 range)
  3 hash mod   mix(key) % R                  ANY R
  4 bounds     #{bounds <= key}              ANY R  (kPartBounds: custom
                                             split points, unsigned compare)
Funcs 2/3 lift the r01 pow2-only restriction. The LDS counter layout
caps ONE kernel pass at 2^12 digits; the writer runs a two-level
coarse/fine pid radix for 4096 < R <= 2^24 (writer._group_pairs_2level).
Func 4 is not a ``PartFunc`` of the hist/scatter/gather kernels: the
search over ``gpu_bounds()`` runs once per record in
extract_pairs_bounds (ops/csrc/bounds.hip), which leaves the partition id
in the pair; the kernels after it run func 0 on that id.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

GPU_MAX_PARTITIONS = 1 << 24
GPU_PART_BOUNDS = 4      # kPartBounds


class HashPartitioner:
    """Multiplicative-mix hash of uint64 keys, modulo num_partitions.

    The mix constant is splitmix64's (0xff51afd7ed558ccd finalizer step) —
    the GPU kernel in ops/csrc/kernels.hip implements the identical
    function so CPU oracle tests compare bit-for-bit.
    """

    MIX = np.uint64(0xFF51AFD7ED558CCD)

    def __init__(self, num_partitions: int):
        self.num_partitions = num_partitions

    def gpu_params(self) -> Optional[Tuple[int, int, int]]:
        R = self.num_partitions
        nbits = (R - 1).bit_length()
        if (1 << nbits) == R and 4 <= nbits <= 12:
            return (1, 0, 0)        # hash then & (R-1) == % R for pow2
        return (3, 0, R)            # hash then % R (any R; the writer
                                    # two-levels when R > 4096)

    def partition_ids(self, keys: np.ndarray) -> np.ndarray:
        k = keys.astype(np.uint64, copy=False)
        with np.errstate(over="ignore"):
            h = (k ^ (k >> np.uint64(33))) * self.MIX
            h ^= h >> np.uint64(33)
        return (h % np.uint64(self.num_partitions)).astype(np.int32)


class RangePartitioner:
    """Range partitioner over uint64 keys — TeraSort's partitioner.

    ``bounds`` are num_partitions-1 ascending split points; partition i
    holds keys in [bounds[i-1], bounds[i]).
    """

    def __init__(self, bounds: np.ndarray):
        self.bounds = np.asarray(bounds, dtype=np.uint64)
        self.num_partitions = len(self.bounds) + 1
        self._uniform_full_range = False

    @classmethod
    def uniform(cls, num_partitions: int,
                key_min: int = 0, key_max: int = 2 ** 64 - 1) -> "RangePartitioner":
        span = (key_max - key_min + 1) if key_max < 2 ** 64 - 1 else 2 ** 64
        # CEILING bounds: partition(key) == floor(key * R / span), exactly
        # the kernel's multiply-high (func 2) for the full-u64 case — so
        # GPU and CPU agree at the boundary keys bit-for-bit
        bounds = [key_min + -(-span * (i + 1) // num_partitions)
                  for i in range(num_partitions - 1)]
        p = cls(np.array(bounds, dtype=np.uint64))
        # pow2 partitions over a pow2 key span starting at 0 => partition
        # id is a plain top-bit shift (func 0)
        nbits = (num_partitions - 1).bit_length()
        if (key_min == 0 and (1 << nbits) == num_partitions
                and span & (span - 1) == 0):
            p.gpu_shift = span.bit_length() - 1 - nbits
        p._uniform_full_range = (key_min == 0 and span == 2 ** 64)
        return p

    @classmethod
    def from_sample(cls, sample, num_partitions: int) -> "RangePartitioner":
        """Split points from a key sample — what TeraSort's sampled
        partitioner and Spark's RangePartitioner (under ``sortByKey``) do.

        ``sample`` is a numpy u64 array or an int64 torch tensor holding
        u64 bits; a device tensor is sorted on the device. Bound i is
        ``sorted_sample[(i+1)*s // R]``. Duplicate bounds are kept: the
        partitions between them are simply empty and R stays what the
        shuffle was registered with."""
        R = int(num_partitions)
        if R < 1:
            raise ValueError("num_partitions must be >= 1")
        if isinstance(sample, np.ndarray):
            srt = np.sort(sample.astype(np.uint64, copy=False).reshape(-1))
            s = len(srt)
        else:
            import torch
            t = sample.reshape(-1)
            if t.dtype != torch.int64:
                raise TypeError("a tensor sample must be int64 (u64 bits)")
            s = t.numel()
            if t.is_cuda and s:
                from .ops.radix import sort_pairs
                srt, _ = sort_pairs(t.clone())      # unsigned order
            else:
                srt = np.sort(t.cpu().numpy().view(np.uint64))
        if s == 0:
            raise ValueError("cannot derive bounds from an empty sample")
        pick = (np.arange(1, R, dtype=np.int64) * s) // R
        if isinstance(srt, np.ndarray):
            bounds = srt[pick]
        else:
            import torch
            bounds = srt[torch.from_numpy(pick).to(srt.device)] \
                .cpu().numpy().view(np.uint64)
        return cls(bounds)

    def gpu_params(self) -> Optional[Tuple[int, int, int]]:
        R = self.num_partitions
        if hasattr(self, "gpu_shift"):
            return (0, self.gpu_shift, 0)
        if self._uniform_full_range:
            return (2, 0, R)        # mulhi(key, R) — any R; the writer
                                    # two-levels when R > 4096
        return (GPU_PART_BOUNDS, 0, R)  # custom bounds: splitter search

    def gpu_bounds(self, device):
        """The bounds as an int64 device tensor (u64 bits), uploaded once
        per device and cached."""
        import torch
        dev = torch.device(device)
        cache: Dict[str, object] = self.__dict__.setdefault(
            "_gpu_bounds", {})
        t = cache.get(str(dev))
        if t is None:
            t = torch.from_numpy(
                np.ascontiguousarray(self.bounds).view(np.int64)).to(dev)
            cache[str(dev)] = t
        return t

    def partition_ids(self, keys: np.ndarray) -> np.ndarray:
        k = keys.astype(np.uint64, copy=False)
        return np.searchsorted(self.bounds, k, side="right").astype(np.int32)


def sample_bounds(engine, local_keys, num_partitions: int,
                  sample_per_rank: int, seed: int = 0) -> RangePartitioner:
    """SPMD-collective: every rank gets the SAME sampled RangePartitioner.

    Each rank draws ``sample_per_rank`` of its keys (numpy u64, or an
    int64 tensor on any device) with a generator seeded by (seed, rank),
    and ships them through the CPU lane of a one-partition shuffle; after
    the barrier every rank reads partition 0 — the union of all samples —
    and derives the bounds from it. No RPC beyond the shuffle's own."""
    n = len(local_keys)
    k = min(int(sample_per_rank), n)
    rng = np.random.default_rng([int(seed), int(engine.rank)])
    idx = np.sort(rng.choice(n, size=k, replace=False)) if k else \
        np.empty(0, dtype=np.int64)
    if isinstance(local_keys, np.ndarray):
        mine = local_keys[idx].astype(np.uint64, copy=False)
    else:
        import torch
        mine = local_keys[torch.from_numpy(idx).to(local_keys.device)] \
            .cpu().numpy().view(np.uint64)
    handle = engine.register_shuffle(engine.world_size, 1)
    w = engine.manager.get_writer(handle, engine.rank)
    w.write_batch(mine)
    w.stop(True, partitioner=RangePartitioner(np.empty(0, dtype=np.uint64)))
    engine.barrier()
    chunks = []
    for _ref, data in engine.manager.get_reader(handle, 0, 0):
        if not isinstance(data, (bytes, bytearray, memoryview)):
            data = data.cpu().numpy().tobytes()   # GPU plane: device arena
        chunks.append(np.frombuffer(bytes(data), dtype="<u8"))
    # barrier (every rank has read) + release of the sample blocks
    engine.unregister_shuffle(handle)
    union = np.concatenate(chunks) if chunks else \
        np.empty(0, dtype=np.uint64)
    return RangePartitioner.from_sample(union, num_partitions)
