"""How a sweep's points are divided: the block split, the cut of a per-point argument to a block, the thread-per-device
runner of ``devices=[...]`` and this process's share under a ``torch.distributed`` process group.  Torch-free: torch is
only touched when a caller has already initialised a process group."""
from __future__ import annotations

import sys
from typing import Optional, Tuple

import numpy as np

# Per-point arguments of each entry point: name -> (axis of the points, ndim of the per-point form).
SWEEP_AXES = {"dbeta": (0, 1), "dbeta2": (0, 1), "gamma": (0, 1), "alpha": (0, 1), "a0": (0, 2)}
PAIRS_AXES = {"dbeta": (0, 2), "gamma": (0, 1), "alpha": (0, 1), "a0": (0, 2)}
COMB_AXES = {"kappa": (0, 2), "gamma": (0, 1), "alpha": (0, 1), "a0": (0, 2)}
CHAIN_AXES = {"dbeta": (1, 2), "dbeta2": (1, 2), "gamma": (1, 2), "alpha": (1, 2), "a0": (0, 2), "transfers": (1, 3)}
PAIRS_CHAIN_AXES = {"dbeta": (1, 3), "gamma": (1, 2), "alpha": (1, 2), "a0": (0, 2), "transfers": (1, 3)}


def shard_bounds(n_points: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block split; the first ``n_points % world`` ranks get one extra point."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad rank/world: {rank}/{world}")
    base, rem = divmod(int(n_points), world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def cut(kw: dict, axes: dict, n: int, sel) -> dict:
    """``kw`` with every per-point argument of the table ``axes`` cut to ``sel`` (a slice or an index array) along its
    axis.  Per-point means the table's ndim with n entries on that axis; scalars, single rows, None and n = 1 pass through."""
    out = dict(kw)
    for name, (axis, ndim) in axes.items():
        x = None if n == 1 else kw.get(name)
        if x is not None:
            x = np.asarray(x)
            if x.ndim == ndim and x.shape[axis] == n:
                out[name] = x[(slice(None),) * axis + (sel,)]
    return out


def over_devices(fn, devices, n: int, axes: dict, kw: dict) -> dict:
    """One host thread per device, each calling ``fn(device=d, **kw)`` on its contiguous block of the n points (ctypes
    drops the GIL for the call; the C-ABI is thread-safe for distinct devices).  Empty blocks are skipped; every array the
    first block returns is concatenated in block order, and elapsed_ms is the slowest block's."""
    from concurrent.futures import ThreadPoolExecutor
    k = len(devices)

    def run(r):
        lo, hi = shard_bounds(n, k, r)
        return fn(device=int(devices[r]), **cut(kw, axes, n, slice(lo, hi))) if hi > lo else None

    with ThreadPoolExecutor(max_workers=k) as pool:
        parts = [p for p in pool.map(run, range(k)) if p is not None]
    out = {key: np.concatenate([p[key] for p in parts]) for key, v in parts[0].items()
           if v is not None and key != "elapsed_ms"}
    out["elapsed_ms"] = max(p["elapsed_ms"] for p in parts)
    return out


class Share:
    """This process's share [lo, hi) of n points under the process group ``group``: all of them (world 1, rank 0) when no
    group is up.  ``width`` is the widest block; ``device`` the GPU this rank drives (``distributed.local_device`` under a
    group unless given)."""

    def __init__(self, n: int, device: Optional[int] = None, group=None):
        self.n, self.group, self.world, self.rank = int(n), group, 1, 0
        td = sys.modules.get("torch.distributed")      # a caller who initialised a process group has imported it
        up = td is not None and td.is_available() and td.is_initialized()
        if up:
            self.world, self.rank = td.get_world_size(group), td.get_rank(group)
        self.lo, self.hi = shard_bounds(self.n, self.world, self.rank)
        self.width = -(-self.n // self.world)
        if device is None and up:
            from .distributed import local_device
            device = local_device(group)
        self.device = 0 if device is None else int(device)

    @property
    def sharded(self) -> bool:
        return self.world > 1
