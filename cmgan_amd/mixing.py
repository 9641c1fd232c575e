"""Dynamic mixing: noisy and reverberant training batches made from clean speech on the GPU (Engine.mix / cmgan_mix).

The reference's data path replays pairs that somebody mixed beforehand (`DemandDataset`: clean/x.wav with noisy/x.wav).
Here a batch needs only clean speech to cross PCIe: noise recordings and room impulse responses live on the device in a
`NoiseBank` / `RirBank`, a `DynamicMixer` draws per-row noise item, offset, SNR and RIR on the device and makes one
`Engine.mix` call, and a `MixingLoader` turns a loader of clean clips into the `(clean, noisy, length)` batches `Trainer`
takes - with `clean` the training target (the dry clip, or the clip with its early reflections).

    noise = NoiseBank.from_dir("noise/", 16000, engine)
    rirs = RirBank.from_dir("rirs/", 16000, engine)
    mixer = DynamicMixer(engine, noise, rirs, snr_db=(0, 20), early_ms=50)
    # without recorded responses: simulate shoe-box rooms on the device (Engine.rir / cmgan_rir, image-source method),
    # either a fixed bank       rirs = RirBank.simulate(engine, RoomSampler(), 256)
    # or a fresh room per row of every batch
    mixer = DynamicMixer(engine, noise, rooms=RoomSampler(rt60=(0.2, 0.8)), snr_db=(0, 20), early_ms=50)
    clean = torch.utils.data.DataLoader(clean_only("data/train", 32000), batch_size=32, pin_memory=True, drop_last=True)
    Trainer(train_ds=MixingLoader(clean, mixer), ...)
"""
from __future__ import annotations

import collections
import math
import os
import random
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.utils.data

from .data import _natural_key, fit_length, read_wav

__all__ = ["NoiseBank", "RirBank", "RoomSampler", "sabine_beta", "DynamicMixer", "MixingLoader", "CleanDataset",
           "clean_only", "Draw", "tile"]

SPEED_OF_SOUND = 343.0        # m/s, the default `c` of Engine.rir
RIR_TW = 40                   # the default half-width of its fractional-delay filter, in samples


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


def sabine_beta(rt60, dims) -> torch.Tensor:
    """The reflection coefficient that gives a shoe-box room of size `dims` ([..., 3], metres) the reverberation time
    `rt60` ([...], seconds) by Sabine's formula: alpha = 0.161 V / (S rt60) clamped to [0, 1], beta = sqrt(1 - alpha), the
    same for all six walls.  Plain tensor arithmetic on the device of its arguments; returns a tensor of rt60's shape."""
    dims = dims if isinstance(dims, torch.Tensor) else torch.as_tensor(dims, dtype=torch.float64)
    rt60 = rt60 if isinstance(rt60, torch.Tensor) else torch.as_tensor(rt60, dtype=dims.dtype, device=dims.device)
    lx, ly, lz = dims[..., 0], dims[..., 1], dims[..., 2]
    volume = lx * ly * lz
    surface = 2.0 * (lx * ly + ly * lz + lx * lz)
    alpha = (0.161 * volume / (surface * rt60)).clamp(0.0, 1.0)
    return torch.sqrt(1.0 - alpha)


class RoomSampler:
    """Random shoe-box rooms for Engine.rir: `draw(R, K, fs)` -> `(rooms float64 [R, 15], n_taps int32 [R])`.

    Per row: the size uniform per axis between `dims` = (low, high) (metres), source and receiver uniform and independent
    in the room shrunk by `margin` on every side, rt60 uniform in `rt60` = (low, high) seconds; the six reflection
    coefficients are `sabine_beta(rt60, size)` and n_taps = min(K, ceil(rt60 fs)).  Everything is drawn from `generator`
    (None: the device's default one) on the device with tensor arithmetic: no host synchronisation."""

    def __init__(self, dims=((3.0, 3.0, 2.5), (10.0, 8.0, 4.0)), rt60=(0.2, 0.8), margin: float = 0.5,
                 generator: Optional[torch.Generator] = None):
        try:
            lo, hi = (tuple(float(v) for v in d) for d in dims)
        except (TypeError, ValueError):
            raise ValueError(f"dims must be ((Lx, Ly, Lz) low, (Lx, Ly, Lz) high), got {dims}") from None
        if len(lo) != 3 or len(hi) != 3 or not all(0.0 < a <= b < math.inf for a, b in zip(lo, hi)):
            raise ValueError(f"dims must be ((Lx, Ly, Lz) low, (Lx, Ly, Lz) high) with 0 < low <= high, got {dims}")
        t_lo, t_hi = float(rt60[0]), float(rt60[1])
        if not 0.0 < t_lo <= t_hi < math.inf:
            raise ValueError(f"rt60 must be (low, high) with 0 < low <= high, got {rt60}")
        margin = float(margin)
        if not 0.0 <= margin < 0.5 * min(lo):
            raise ValueError(f"margin must lie in [0, {0.5 * min(lo)}): half the smallest room size of {dims}, got {margin}")
        self.lo, self.hi, self.rt60, self.margin, self.generator = lo, hi, (t_lo, t_hi), margin, generator

    def n_images(self, K: int, fs: int, c: float = SPEED_OF_SOUND, tw: int = RIR_TW):
        """(Nx, Ny, Nz) that leaves out no image of a K-tap response in any room this sampler draws: host arithmetic on
        the LOWER size bound, ceil((K + tw) c / fs / (2 Lmin_axis)) + 1."""
        return tuple(int(math.ceil((K + tw) * c / fs / (2.0 * l))) + 1 for l in self.lo)

    def draw(self, R: int, K: int, fs: int, device=None):
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        u = torch.rand(R, 10, dtype=torch.float64, generator=gen, device=device)
        lo = torch.tensor(self.lo, dtype=torch.float64).to(device, non_blocking=True)
        hi = torch.tensor(self.hi, dtype=torch.float64).to(device, non_blocking=True)
        size = lo + (hi - lo) * u[:, 0:3]
        inner = size - 2.0 * self.margin
        source = self.margin + inner * u[:, 3:6]
        receiver = self.margin + inner * u[:, 6:9]
        rt = self.rt60[0] + (self.rt60[1] - self.rt60[0]) * u[:, 9]
        beta = sabine_beta(rt, size)
        rooms = torch.cat([size, source, receiver, beta[:, None].expand(R, 6)], dim=1).contiguous()
        n_taps = torch.ceil(rt * fs).clamp(1, K).to(torch.int32)
        return rooms, n_taps


class RirBank:
    """Room impulse responses as one float32 [R, Kmax] device allocation, rows zero-padded, plus `length` (int32 [R]).
    Recorded responses come from `from_dir` / `from_arrays`; `simulate` makes the bank on the device from random shoe-box
    rooms (Engine.rir, the image-source method) and keeps their table as `rooms` (float64 [R, 15], else None)."""

    def __init__(self, data: torch.Tensor, length: torch.Tensor, rooms: Optional[torch.Tensor] = None):
        self.data, self.length, self.rooms = data, length, rooms

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

    @classmethod
    def simulate(cls, engine, sampler: RoomSampler, R: int, seconds: float = 0.5, sample_rate: int = 16000) -> "RirBank":
        """R rooms drawn by `sampler`, each simulated for up to `seconds` (a row's own length is its rt60, if shorter)."""
        K = int(round(seconds * sample_rate))
        rooms, n_taps = sampler.draw(R, K, sample_rate, device=engine.device)
        data, length = engine.rir(rooms, n_taps, K, sampler.n_images(K, sample_rate), fs=sample_rate)
        return cls(data, length, rooms)

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
    rooms: Optional[torch.Tensor] = None      # DynamicMixer(rooms=...): the float64 [B, 15] room table of the batch
    level_db: Optional[torch.Tensor] = None   # DynamicMixer(level_db=...): the float64 [B] target active level in dBFS


class DynamicMixer:
    """`mixer(clean_dev)` -> `(target, noisy, MixInfo)` for a float32 [B, L] device batch of clean speech.

    Per row and per call it draws, on the device and from `generator` (a torch.Generator of the engine's device; None
    uses the device's default one): a noise item (uniform), an offset into it (uniform), an SNR uniform in `snr_db` =
    (lo, hi) dB and, with a `rir_bank`, a RIR (uniform; with probability 1 - p_reverb the row gets the one-tap identity
    appended to the bank instead).  `early_ms`: the target keeps that much of the RIR after its direct path (the usual
    dereverberation target); None makes the dry clip the target.  Nothing here synchronises with the host; the draws of
    the last call stay readable as `mixer.last_draw`.

    `rooms` (a RoomSampler, instead of a `rir_bank`) gives every row of every call a room of its own: B rooms are drawn
    and simulated for `rir_seconds` by Engine.rir into one persistent [B (+ 1), K] allocation, row b uses response b
    (rir_index = arange(B)), and with p_reverb < 1 the dry rows use the identity appended as row B.  The room draws come
    from the sampler's own generator, after the mixer's; the bank of the last call stays readable as `mixer.last_bank`
    (the next call overwrites it in place).

    Levels (Engine.speech_level / cmgan_speech_level: the active speech level of ITU-T P.56, method B).  Either option
    below measures the clean batch once per call, on the device; the measurement stays readable as `mixer.last_level`.
    With both at their defaults nothing is measured, no draw is added and the outputs are what they were without them.
    `snr_on="active"`: the drawn SNR relates the ACTIVE speech power to the noise power, as speech corpora define it: the
    mixer passes snr_db - D to Engine.mix, D = -10 log10(activity) where the row's activity is finite and > 0, else 0
    ("rms", the default: mean(speech^2) over the whole clip, pauses included).  `last_draw.snr_db` stays the drawn value.
    D is measured on the dry clip; with a RIR the reverberant speech's own activity differs slightly.
    `level_db=(lo, hi)`: a target active level, uniform in dBFS, is drawn per row (after every other draw) and the clean
    row is multiplied in float32 by f32(sqrt(10^(level / 10) / active_ms)) before Engine.mix; the factor is 1 where no
    speech was detected.  This is one measurement and one gain: the thresholds of P.56 are absolute, so measuring the
    scaled row again gives a slightly different level than the one drawn."""

    def __init__(self, engine, noise_bank: NoiseBank, rir_bank: Optional[RirBank] = None, snr_db=(0.0, 20.0),
                 early_ms: Optional[float] = 50.0, p_reverb: float = 1.0, peak: float = 0.99,
                 generator: Optional[torch.Generator] = None, sample_rate: int = 16000,
                 rooms: Optional[RoomSampler] = None, rir_seconds: float = 0.5, snr_on: str = "rms", level_db=None):
        if snr_on not in ("rms", "active"):
            raise ValueError(f"snr_on must be 'rms' or 'active', got {snr_on!r}")
        if level_db is not None:
            try:
                level_db = (float(level_db[0]), float(level_db[1]))
            except (TypeError, ValueError, IndexError):
                raise ValueError(f"level_db must be None or (low, high) in dBFS, got {level_db}") from None
            if not level_db[0] <= level_db[1] < math.inf or level_db[0] == -math.inf:
                raise ValueError(f"level_db must be (low, high) with finite low <= high, got {level_db}")
        if (snr_on == "active" or level_db is not None) and not 8000 <= int(sample_rate) <= 192000:
            raise ValueError(f"the speech level is measured at 8000 .. 192000 Hz, got sample_rate = {sample_rate}")
        self.snr_on, self.level_db, self.last_level = snr_on, level_db, None
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
        self.rooms, self.sample_rate = rooms, int(sample_rate)
        self.rir_taps, self.n_images, self.last_bank = 0, None, None
        if rooms is not None:
            if rir_bank is not None:
                raise ValueError("give either a rir_bank or rooms, not both")
            self.rir_taps = int(round(rir_seconds * sample_rate))
            if not 1 <= self.rir_taps <= 65536:
                raise ValueError(f"rir_seconds must give 1 .. 65536 taps, got {rir_seconds} s at {sample_rate} Hz")
            self.n_images = rooms.n_images(self.rir_taps, self.sample_rate)
            if max(self.n_images) > 255:
                raise ValueError(f"responses of {rir_seconds} s in rooms as small as {rooms.lo} need image ranges "
                                 f"{self.n_images}; up to 255 are supported")

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
        table = None
        if self.rooms is not None:
            table, rlen = self.rooms.draw(B, self.rir_taps, self.sample_rate, device=dev)
            idx = torch.arange(B, dtype=torch.int32, device=dev)
            if self.p_reverb < 1.0:
                wet = torch.rand(B, dtype=torch.float32, generator=gen, device=dev) < self.p_reverb
                idx = torch.where(wet, idx, torch.full_like(idx, B))
                rlen = torch.where(wet, rlen, torch.ones_like(rlen))
        level = None
        if self.level_db is not None:
            lo, hi = self.level_db
            level = lo + (hi - lo) * torch.rand(B, dtype=torch.float64, generator=gen, device=dev)
        return Draw(start.contiguous(), length.contiguous(), off, snr, idx, rlen, table, level)

    def _simulate(self, d: Draw) -> RirBank:
        """The batch's responses, simulated into the persistent allocation (made anew only when B changes)."""
        B, K = d.rooms.size(0), self.rir_taps
        rows = B + (1 if self.p_reverb < 1.0 else 0)
        if self.last_bank is None or self.last_bank.data.size(0) != rows:
            data = torch.zeros(rows, K, dtype=torch.float32, device=self.engine.device)
            length = torch.ones(rows, dtype=torch.int32, device=self.engine.device)
            if rows > B:
                data[B, 0] = 1.0                                  # the identity of the dry rows
            self.last_bank = RirBank(data, length)
        sim = self.last_bank
        # rir_len is the sampler's n_taps, or 1 for a dry row (whose response is then one tap that no row uses)
        self.engine.rir(d.rooms, d.rir_len, K, self.n_images, fs=self.sample_rate, out=(sim.data[:B], sim.length[:B]))
        return sim

    @staticmethod
    def level_gain(level, level_db: torch.Tensor) -> torch.Tensor:
        """The float32 [B] factor that takes rows measured as `level` (a SpeechLevel) to the active level `level_db`
        (float64 [B], dBFS): f32(sqrt(10^(level_db / 10) / active_ms)), and 1 where active_ms is not finite and > 0."""
        ok = torch.isfinite(level.active_ms) & (level.active_ms > 0)
        active = torch.where(ok, level.active_ms, torch.ones_like(level.active_ms))
        gain = torch.sqrt(torch.pow(10.0, level_db / 10.0) / active)
        return torch.where(ok, gain, torch.ones_like(gain)).to(torch.float32)

    def __call__(self, clean: torch.Tensor):
        d = self.last_draw = self.draw(clean.size(0))
        rir = self.rir_bank if self.rooms is None else self._simulate(d)
        snr = d.snr_db
        if self.snr_on == "active" or d.level_db is not None:
            lv = self.last_level = self.engine.speech_level(clean, fs=self.sample_rate)
            if self.snr_on == "active":
                ok = torch.isfinite(lv.activity) & (lv.activity > 0)
                delta = torch.where(ok, -10.0 * torch.log10(torch.where(ok, lv.activity, torch.ones_like(lv.activity))),
                                    torch.zeros_like(lv.activity))
                snr = (d.snr_db.to(torch.float64) - delta).to(torch.float32).contiguous()
            if d.level_db is not None:
                clean = (clean * self.level_gain(lv, d.level_db)[:, None]).contiguous()
        noisy, target, info = self.engine.mix(clean, self.noise_bank.data, d.noise_start, d.noise_len, d.noise_off,
                                              snr, rir.data if rir is not None else None, d.rir_index, d.rir_len,
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
