"""DeviceGenerator: the counter-based normal generator of the device (csrc/philox.h, include/avsd.h "random numbers") as an object.

A draw is a pure function of (seed, stream, step, element index): Philox4x32-10 plus Box-Muller in f32 and integers only.  The
generator's whole state is therefore the seed and how many streams it has handed out; the same seed and the same order of calls
give the same bits on any machine and in either build of the library.  A stream is one independent sequence (the initial noise
of one clip, say); `step` is a second index inside a stream, meant for the steps of a sampling run.  The pipeline's `noise=`
argument takes what `normal()` returns.

It is not bit-compatible with `torch.randn` on any device, and is not meant to be."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


class DeviceGenerator:
    def __init__(self, seed: int = 0):
        self.manual_seed(seed)

    def manual_seed(self, seed: int) -> "DeviceGenerator":
        """resets the seed and the count of streams handed out"""
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an unsigned 64-bit integer, got {seed}")
        self.seed = seed
        self.streams = 0
        return self

    def initial_seed(self) -> int:
        return self.seed

    def next_stream(self) -> int:
        """a fresh 32-bit stream id"""
        if self.streams >= 1 << 32:
            raise RuntimeError("DeviceGenerator: all 2^32 streams of this seed are used; reseed")
        s = self.streams
        self.streams += 1
        return s

    def take_streams(self, n: int) -> int:
        """`n` consecutive fresh stream ids; returns the first.  A stochastic sampler takes one per batch row of a clip and draws
        row b's noise of step i as (stream + b, step i)."""
        n = int(n)
        if n < 0 or self.streams + n > 1 << 32:
            raise RuntimeError(f"DeviceGenerator: {n} more streams are not left in the 2^32 of this seed; reseed")
        s = self.streams
        self.streams += n
        return s

    def normal(self, shape, device="cuda", stream: Optional[int] = None, step: int = 0) -> torch.Tensor:
        """f32 normals of `shape` on `device`: element i (row-major) is normal i of (seed, stream, step); `stream=None` takes a
        fresh stream"""
        if stream is None:
            stream = self.next_stream()
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for d in shape:
            n *= d
        return ops.randn_philox(n, self.seed, stream, step, 0, device=device).reshape(shape)
