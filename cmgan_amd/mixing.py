"""Dynamic mixing: noisy and reverberant training batches made from clean speech on the GPU (Engine.mix / cmgan_mix).

The reference's data path replays pairs that somebody mixed beforehand (`DemandDataset`: clean/x.wav with noisy/x.wav).
Here a batch needs only clean speech to cross PCIe: noise recordings and room impulse responses live on the device in a
`NoiseBank` / `RirBank`, a `DynamicMixer` draws per-row noise item, offset, SNR and RIR on the device and makes one
`Engine.mix` call, and a `MixingLoader` turns a loader of clean clips into the `(clean, noisy, length)` batches `Trainer`
takes - with `clean` the training target (the dry clip, or the clip with its early reflections).

    noise = NoiseBank.from_dir("noise/", 16000, engine)
    rirs = RirBank.from_dir("rirs/", 16000, engine)
    mixer = DynamicMixer(engine, noise, rirs, snr_db=(0, 20), early_ms=50)
    clean = torch.utils.data.DataLoader(clean_only("data/train", 32000), batch_size=32, pin_memory=True, drop_last=True)
    Trainer(train_ds=MixingLoader(clean, mixer), ...)
"""
from __future__ import annotations

import collections
import os
import random
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.utils.data

from .data import _natural_key, fit_length, read_wav

__all__ = ["NoiseBank", "RirBank", "DynamicMixer", "MixingLoader", "CleanDataset", "clean_only", "Draw", "tile"]


def tile() -> int:
    """Samples per block of the mixing kernels (cmgan_mix_tile): the granularity of their fixed-order reductions."""
    from . import _lib
    return int(_lib.load().cmgan_mix_tile())


def _as_rows(arrays: Sequence) -> list:
    rows = []
    for k, a in enumerate(arrays):
        t = torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).detach().to(torch.float32)
        if t.dim() != 1 or t.numel() < 1:
            raise ValueError(f"item {k}: expected a 1-D array with at least one sample, got {tuple(t.shape)}")
        rows.append(t)
    if not rows:
        raise ValueError("a bank needs at least one item")
    return rows


def _read_dir(path: str, sample_rate: int, engine) -> list:
    names = sorted((n for n in os.listdir(path) if n.lower().endswith(".wav")), key=_natural_key)
    if not names:
        raise ValueError(f"{path}: no .wav files")
    rows = []
    for n in names:
        x, sr = read_wav(os.path.join(path, n))
        x = x.to(engine.device)
        if sr != sample_rate:
            x = engine.resample(x, sr, sample_rate)
        rows.append(x)
    return rows


class NoiseBank:
    """Noise recordings of any lengths as ONE flat float32 device allocation plus index tables: `start` / `length`
    (int64 [items]) say where item k lies in `data`."""

    def __init__(self, data: torch.Tensor, start: torch.Tensor, length: torch.Tensor):
        self.data, self.start, self.length = data, start, length

    def __len__(self) -> int:
        return self.start.numel()

    @property
    def device(self) -> torch.device:
        return self.data.device

    @classmethod
    def from_arrays(cls, arrays: Sequence, device=None) -> "NoiseBank":
        rows = _as_rows(arrays)
        device = torch.device(device) if device is not None else rows[0].device
        lens = [r.numel() for r in rows]
        data = torch.cat([r.to(device) for r in rows]).contiguous()
        length = torch.tensor(lens, dtype=torch.int64)
        start = torch.cumsum(length, 0) - length
        return cls(data, start.to(device), length.to(device))

    @classmethod
    def from_dir(cls, path: str, sample_rate: int, engine) -> "NoiseBank":
        """Every .wav under `path` (natural order); files at another rate go through Engine.resample."""
        return cls.from_arrays(_read_dir(path, sample_rate, engine), device=engine.device)


class RirBank:
    """Room impulse responses as one float32 [R, Kmax] device allocation, rows zero-padded, plus `length` (int32 [R])."""

    def __init__(self, data: torch.Tensor, length: torch.Tensor):
        self.data, self.length = data, length

    def __len__(self) -> int:
        return self.data.size(0)

    @property
    def device(self) -> torch.device:
        return self.data.device

    @classmethod
    def from_arrays(cls, arrays: Sequence, device=None) -> "RirBank":
        rows = _as_rows(arrays)
        device = torch.device(device) if device is not None else rows[0].device
        kmax = max(r.numel() for r in rows)
        data = torch.zeros(len(rows), kmax, dtype=torch.float32, device=device)
        for k, r in enumerate(rows):
            data[k, :r.numel()] = r.to(device)
        return cls(data, torch.tensor([r.numel() for r in rows], dtype=torch.int32).to(device))

    @classmethod
    def from_dir(cls, path: str, sample_rate: int, engine) -> "RirBank":
        return cls.from_arrays(_read_dir(path, sample_rate, engine), device=engine.device)

    def with_identity(self) -> "RirBank":
        """The bank with a one-tap identity response appended as its last row (rows that get no reverberation)."""
        row = torch.zeros(1, self.data.size(1), dtype=torch.float32, device=self.device)
        row[0, 0] = 1.0
        one = torch.ones(1, dtype=torch.int32, device=self.device)
        return RirBank(torch.cat([self.data, row]).contiguous(), torch.cat([self.length, one]))


class Draw(NamedTuple):
    """What a DynamicMixer drew for a batch: device tensors [B], exactly the per-row arguments of Engine.mix."""
    noise_start: torch.Tensor
    noise_len: torch.Tensor
    noise_off: torch.Tensor
    snr_db: torch.Tensor
    rir_index: Optional[torch.Tensor]
    rir_len: Optional[torch.Tensor]


class DynamicMixer:
    """`mixer(clean_dev)` -> `(target, noisy, MixInfo)` for a float32 [B, L] device batch of clean speech.

    Per row and per call it draws, on the device and from `generator` (a torch.Generator of the engine's device; None
    uses the device's default one): a noise item (uniform), an offset into it (uniform), an SNR uniform in `snr_db` =
    (lo, hi) dB and, with a `rir_bank`, a RIR (uniform; with probability 1 - p_reverb the row gets the one-tap identity
    appended to the bank instead).  `early_ms`: the target keeps that much of the RIR after its direct path (the usual
    dereverberation target); None makes the dry clip the target.  Nothing here synchronises with the host; the draws of
    the last call stay readable as `mixer.last_draw`."""

    def __init__(self, engine, noise_bank: NoiseBank, rir_bank: Optional[RirBank] = None, snr_db=(0.0, 20.0),
                 early_ms: Optional[float] = 50.0, p_reverb: float = 1.0, peak: float = 0.99,
                 generator: Optional[torch.Generator] = None, sample_rate: int = 16000):
        lo, hi = float(snr_db[0]), float(snr_db[1])
        if not lo <= hi:
            raise ValueError(f"snr_db must be (low, high) with low <= high, got {snr_db}")
        if not 0.0 <= p_reverb <= 1.0:
            raise ValueError(f"p_reverb must lie in [0, 1], got {p_reverb}")
        if early_ms is not None and early_ms < 0:
            raise ValueError(f"early_ms must be >= 0 or None, got {early_ms}")
        for name, bank in (("noise_bank", noise_bank), ("rir_bank", rir_bank)):
            if bank is not None and bank.device != engine.device:
                raise RuntimeError(f"{name} is on {bank.device} but the engine is bound to {engine.device}")
        self.engine, self.noise_bank, self.snr_db, self.peak = engine, noise_bank, (lo, hi), float(peak)
        self.p_reverb, self.generator = float(p_reverb), generator
        self.n_rirs = len(rir_bank) if rir_bank is not None else 0
        self.rir_bank = rir_bank.with_identity() if rir_bank is not None and p_reverb < 1.0 else rir_bank
        self.early = -1 if early_ms is None else int(round(early_ms * sample_rate / 1000.0))
        self.last_draw: Optional[Draw] = None

    def draw(self, B: int) -> Draw:
        dev, gen, nb = self.engine.device, self.generator, self.noise_bank
        item = torch.randint(0, len(nb), (B,), generator=gen, device=dev)
        start, length = nb.start[item], nb.length[item]
        u = torch.rand(B, dtype=torch.float64, generator=gen, device=dev)
        off = torch.minimum((u * length).to(torch.int64), length - 1)
        lo, hi = self.snr_db
        snr = (lo + (hi - lo) * torch.rand(B, dtype=torch.float32, generator=gen, device=dev)).contiguous()
        idx = rlen = None
        if self.rir_bank is not None:
            idx = torch.randint(0, self.n_rirs, (B,), generator=gen, device=dev)
            if self.p_reverb < 1.0:
                wet = torch.rand(B, dtype=torch.float32, generator=gen, device=dev) < self.p_reverb
                idx = torch.where(wet, idx, torch.full_like(idx, self.n_rirs))
            rlen = self.rir_bank.length[idx].contiguous()
            idx = idx.to(torch.int32)
        return Draw(start.contiguous(), length.contiguous(), off, snr, idx, rlen)

    def __call__(self, clean: torch.Tensor):
        d = self.last_draw = self.draw(clean.size(0))
        rir = self.rir_bank
        noisy, target, info = self.engine.mix(clean, self.noise_bank.data, d.noise_start, d.noise_len, d.noise_off,
                                              d.snr_db, rir.data if rir is not None else None, d.rir_index, d.rir_len,
                                              peak=self.peak, early=self.early if rir is not None else -1)
        return target, noisy, info


class CleanDataset(torch.utils.data.Dataset):
    """The clean/ half of `DemandDataset`: `<data_dir>/clean/*.wav` in natural order, items `(clean, length)` with the
    same length rule (short clips repeated, long ones cropped at `random.randint(0, length - cut_len)`)."""

    def __init__(self, data_dir: str, cut_len: int = 16000 * 2):
        self.cut_len = cut_len
        self.clean_dir = os.path.join(data_dir, "clean")
        self.clean_wav_name = sorted(os.listdir(self.clean_dir), key=_natural_key)

    def __len__(self) -> int:
        return len(self.clean_wav_name)

    def __getitem__(self, idx: int):
        clean, _ = read_wav(os.path.join(self.clean_dir, self.clean_wav_name[idx]))
        length = clean.numel()
        start = random.randint(0, length - self.cut_len) if length >= self.cut_len else 0
        return fit_length(clean, self.cut_len, start), length


def clean_only(data_dir: str, cut_len: int = 16000 * 2) -> CleanDataset:
    return CleanDataset(data_dir, cut_len)


class MixingLoader:
    """Wraps a loader of clean clips - batches `(clean [B, L], length [B])`, or any tuple whose first element is the
    clean batch and whose last is the lengths - and yields `(target, noisy, length)` with target / noisy float32 device
    tensors: the `(clean, noisy, length)` batches of `load_data`, so `Trainer(train_ds=MixingLoader(...))` works as is.

    Stream ordering.  The clean batch is copied to the device (non-blocking from pinned memory) and mixed on the stream
    that is CURRENT when the batch is requested.  `DevicePrefetcher._stage` requests a batch on the compute stream, then
    makes its side stream wait for the compute stream before it copies the batch into its slot, so that copy is ordered
    behind the mixing kernels.  What it does NOT order is the life of our tensors: the copy is still pending on the side
    stream when `_stage` drops its references, and memory returned to the allocator then would be handed to the next
    kernels of the compute stream.  The loader therefore keeps the tensors of its last three batches alive.  The
    prefetcher waits for batch k's copy on the compute stream before it yields batch k, which is before it requests
    batch k + 2; batch k's tensors are released when batch k + 3 is requested, and those of an epoch's last batches
    stay until the next epoch's batches displace them."""

    def __init__(self, clean_loader, mixer: DynamicMixer):
        self.loader, self.mixer = clean_loader, mixer
        self._alive = collections.deque(maxlen=3)
        self.last_info = None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        dev = self.mixer.engine.device
        for batch in self.loader:
            if isinstance(batch, torch.Tensor):
                clean, length = batch, torch.full((batch.size(0),), batch.size(-1), dtype=torch.int64)
            else:
                clean, length = batch[0], batch[-1]
            clean = clean.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
            target, noisy, info = self.mixer(clean)
            self._alive.append((clean, target, noisy, info, self.mixer.last_draw))
            self.last_info = info
            yield target, noisy, length
