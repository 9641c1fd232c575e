"""Sample-rate conversion in front of and behind the model (cmgan_resample, cmgan_amd/csrc/resample.hip).

The reference asserts ``sr == 16000`` (src/evaluation.py:19) and leaves resampling to the user.  Here a track at any
supported rate is brought to the model's rate on the device, with the arithmetic of
``scipy.signal.resample_poly(x, up, down)`` (default window, ``padtype='constant'``):

    g = gcd(fs_in, fs_out), up = fs_out / g, down = fs_in / g, m = max(up, down), half_len = 10 m
    h = firwin(2 half_len + 1, 1 / m, window=('kaiser', 5.0)) * up, pre = down - half_len % down zeros in front
    pre_remove = (half_len + pre) / down,  N = ceil(L up / down)
    y[n] = sum_i x[i] h[(n + pre_remove) down - i up]

`Engine.resample` converts whole signals.  `Resampler` is the incremental form for live audio: the kernel computes any
range of outputs from a buffer that holds part of the signal, and a sample the buffer lacks counts as zero, which leaves
the float64 sum unchanged; so the concatenated pushes equal the whole-signal call bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib

__all__ = ["Geometry", "geometry", "out_len", "ResamplePlan", "Resampler"]


class Geometry(NamedTuple):
    up: int
    down: int
    n_taps: int          # taps including the zero pre-pad
    pre_remove: int


def geometry(fs_in: int, fs_out: int) -> Geometry:
    """(up, down, n_taps, pre_remove) of a rate pair (cmgan_resample_geometry; host arithmetic, needs no GPU)."""
    v = [ctypes.c_int() for _ in range(4)]
    rc = _lib.load().cmgan_resample_geometry(int(fs_in), int(fs_out), *(ctypes.byref(c) for c in v))
    _lib.check(None, rc)
    return Geometry(*(c.value for c in v))


def out_len(fs_in: int, fs_out: int, n_in: int) -> int:
    """ceil(n_in up / down): the length resample_poly gives n_in samples."""
    n = int(_lib.load().cmgan_resample_out_len(int(fs_in), int(fs_out), int(n_in)))
    if n < 0:
        geometry(fs_in, fs_out)                      # raises with the library's message for an unsupported pair
        raise ValueError(f"n_in must be >= 0, got {n_in}")
    return n


class ResamplePlan:
    """Host bookkeeping of an incremental resampler: which outputs are final after a push and which inputs must stay.
    Pure Python (no torch): tests/test_resample_host.py replays it on index arrays.

    Output n reads inputs ceil(((n + pre_remove) down - (n_taps - 1)) / up) .. floor((n + pre_remove) down / up); it is
    final once the last of them has arrived."""

    def __init__(self, up: int, down: int, n_taps: int, pre_remove: int):
        self.up, self.down, self.n_taps, self.pre_remove = up, down, n_taps, pre_remove
        self.n_in = 0            # inputs received
        self.n_out = 0           # outputs emitted
        self.lo = 0              # first input still held
        self.closed = False

    def first_input(self, n: int) -> int:
        """Oldest input output n reads (clamped to the start of the signal)."""
        return max(-((-((n + self.pre_remove) * self.down - (self.n_taps - 1))) // self.up), 0)

    def last_input(self, n: int) -> int:
        return (n + self.pre_remove) * self.down // self.up

    def plan(self, n_new: int, last: bool = False) -> dict:
        """Step that takes `n_new` more inputs: outputs [n0, n0 + n_out) are computed from the held inputs
        [pos_in, pos_in + n_buf), after which the first `drop` of them are shed."""
        if self.closed:
            raise RuntimeError("stream already flushed")
        if n_new < 0:
            raise ValueError("n_new must be >= 0")
        n_in = self.n_in + n_new
        total = -(-n_in * self.up // self.down)                  # N of the signal so far
        end = total if last else max(total - self.pre_remove, 0)
        end = max(end, self.n_out)
        keep = n_in if last else min(self.first_input(end), n_in)
        return dict(n0=self.n_out, n_out=end - self.n_out, pos_in=self.lo, n_buf=n_in - self.lo,
                    drop=max(keep - self.lo, 0), n_in=n_in, last=bool(last))

    def commit(self, p: dict):
        self.n_in = p["n_in"]
        self.n_out = p["n0"] + p["n_out"]
        self.lo += p["drop"]
        self.closed = p["last"]


class Resampler:
    """Incremental `Engine.resample` for B streams in lock-step: `push(x[B, n])` returns the outputs that are final by
    then ([B, k], k may be 0), `flush()` the rest.  Only the input history the next outputs can still reach is kept.  For
    any chunking the concatenated results equal `engine.resample` of the whole signal bit for bit."""

    def __init__(self, engine, fs_in: int, fs_out: int, B: int = 1):
        self.eng, self.fs_in, self.fs_out, self.B = engine, int(fs_in), int(fs_out), int(B)
        self.geom = geometry(fs_in, fs_out)
        # (equal rates are a copy: output n is input n, nothing to wait for or to keep)
        self.cur = ResamplePlan(*self.geom) if self.geom[:2] != (1, 1) else ResamplePlan(1, 1, 1, 0)
        self.buf = torch.empty(self.B, 0, dtype=torch.float32, device=engine.device)

    n_in = property(lambda self: self.cur.n_in)
    n_out = property(lambda self: self.cur.n_out)

    def _step(self, x: torch.Tensor | None, last: bool) -> torch.Tensor:
        if x is not None:
            x = x.to(device=self.eng.device, dtype=torch.float32)
            if x.dim() == 1:
                x = x[None]
            if x.dim() != 2 or x.size(0) != self.B:
                raise ValueError(f"expected [{self.B}, n] samples, got {tuple(x.shape)}")
            self.buf = torch.cat([self.buf, x], dim=1)
        p = self.cur.plan(0 if x is None else x.size(1), last)
        out = self.eng.resample_chunk(self.buf, p["pos_in"], self.fs_in, self.fs_out, p["n0"], p["n_out"])
        if p["drop"]:
            self.buf = self.buf[:, p["drop"]:].contiguous()
        self.cur.commit(p)
        return out

    @torch.no_grad()
    def push(self, x: torch.Tensor) -> torch.Tensor:
        return self._step(x, False)

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        if self.cur.closed:
            return torch.empty(self.B, 0, dtype=torch.float32, device=self.eng.device)
        return self._step(None, True)
