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
    # what the rooms came out as (Engine.rir_stats / cmgan_rir_stats: T30, DRR, C50, ... per response, on the device):
    # a bank measured and selected by it, or every batch labelled with the acoustics it was mixed with
    rirs = RirBank.simulate(engine, RoomSampler(), 256, measure=True).where(t30=(0.3, 0.6), drr_db=(-5.0, 10.0))
    mixer = DynamicMixer(engine, noise, rooms=RoomSampler(), room_stats=True)      # -> mixer.last_room_stats
    # rooms whose reverberation time falls with frequency: walls that absorb more per octave (tilt) and air absorption
    # (air: the caller's ranges of nepers per metre, one per band), in 7 octave bands (Engine.rir_bands / cmgan_rir_bands)
    mixer = DynamicMixer(engine, noise, rooms=RoomSampler(bands=7, tilt=(0.0, 0.5), air=my_air_ranges), snr_db=(0, 20))
    # long responses - halls, stairwells: the image-source method only to 80 ms after the direct sound, a diffuse tail of
    # decaying noise at the room's decay time from there on (Engine.rir_tail / cmgan_rir_tail)
    mixer = DynamicMixer(engine, noise, rooms=RoomSampler(rt60=(0.4, 1.2), tail_ms=80.0), rir_seconds=1.0)
    # talkers that walk: a path of responses per row, cross-faded by emission time (Engine.scene_path / cmgan_scene_path);
    # with tail_ms the 9 responses per row of a 2 s batch cost little beside the mix itself
    mixer = DynamicMixer(engine, noise, rooms=RoomSampler(tail_ms=80.0), rir_seconds=1.0, motion=(0.5, 1.5), p_motion=0.5)
    # no recorded noise at all: every row of every batch a fresh synthetic noise - spectrum, modulation, hum and clicks of
    # its own (Engine.noise / cmgan_noise); or a fixed bank of it
    mixer = DynamicMixer(engine, None, rirs, noise=NoiseSampler(slope_db=(-9, 3), p_hum=0.2, p_clicks=0.1))
    noise = NoiseBank.synthesize(engine, NoiseSampler(), items=256, seconds=10.0)
    # the recording channel: a random equaliser, a band limit and clipping per row (Engine.channel / cmgan_channel)
    mixer = DynamicMixer(engine, noise, rirs, channel=ChannelSampler(p_bandlimit=0.2, p_clip=0.1))
    clean = torch.utils.data.DataLoader(clean_only("data/train", 32000), batch_size=32, pin_memory=True, drop_last=True)
    Trainer(train_ds=MixingLoader(clean, mixer), ...)
    # speed perturbation: every row resampled by a rate of its own (Engine.warp / cmgan_warp).  The batch comes out
    # warp_len(L, hi) samples long, so the loader cuts clips hi times longer than the batch it wants
    mixer = DynamicMixer(engine, noise, rirs, speed=(0.9, 1.1))
    clean = torch.utils.data.DataLoader(clean_only("data/train", cut_len=math.ceil(32000 * 1.1)), batch_size=32, ...)
    # tempo and pitch perturbation: a time stretch that keeps the pitch (Engine.stretch / cmgan_stretch, WSOLA), and that
    # stretch followed by a warp.  stretch_len(L, tempo=, pitch=, speed=) is the batch length clips of L samples give
    mixer = DynamicMixer(engine, noise, rirs, tempo=(0.9, 1.1), pitch=(-2, 2))
    # the link behind the recording device: G.711 or 16-bit PCM, bursts of lost packets, and a receiver that conceals them
    # by repeating the last pitch period or leaves gaps (Engine.transmit / cmgan_transmit): the last stage of the chain
    mixer = DynamicMixer(engine, noise, rirs, transmission=TransmissionSampler(p=0.5, loss=(0.01, 0.2), burst=(1.0, 4.0)))
    # the device's own noise suppressor (Wiener, spectral subtraction or log-MMSE; Engine.suppress / cmgan_suppress), between
    # the channel and the link
    mixer = DynamicMixer(engine, noise, rirs, suppressor=SuppressorSampler(p=0.5, floor_db=(-25.0, -6.0)))
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
from .engine import (RIR_TAIL_MAX_WINDOW, SCENE_MAX_HOP, SCENE_MAX_WAYPOINTS, STRETCH_HOP, STRETCH_SEARCH, SUPPRESS_MAX_WINDOW,
                     SUPPRESS_N_FFT, SUPPRESS_RULES, RirStats, RirTail, _whole_in, transmit_scalars)

__all__ = ["NoiseBank", "NoiseSampler", "NoiseDraw", "noise_fir", "power_law_magnitude", "RirBank", "RoomSampler", "sabine_beta", "octave_filterbank", "DynamicMixer", "MixingLoader", "CleanDataset",
           "clean_only", "Draw", "SceneDraw", "tile", "ChannelSampler", "biquad_peaking", "biquad_low_shelf", "biquad_high_shelf",
           "biquad_lowpass", "biquad_highpass", "butter_lowpass_sos", "warp_len", "stretch_len", "StretchDraw", "TailDraw", "PathDraw",
           "TransmissionSampler", "TransmitDraw", "TransmitInfo", "SuppressorSampler", "SuppressDraw", "suppress_params", "suppress_n_fft"]

SPEED_OF_SOUND = 343.0        # m/s, the default `c` of Engine.rir
RIR_TW = 40                   # the default half-width of its fractional-delay filter, in samples
SPEED_RANGE = (0.25, 4.0)     # the rates Engine.warp takes (cmgan_warp_max_rate)
THREE_LN10 = 3.0 * math.log(10.0)    # a 60 dB decay over T seconds is 3 ln 10 / T amplitude nepers per second


def warp_len(L: int, rate: float) -> int:
    """How many samples Engine.warp makes of a row of L at `rate` (cmgan_warp_out_len): #{i >= 0 : fl(i rate) < L}."""
    from . import _lib
    n = int(_lib.load().cmgan_warp_out_len(int(L), float(rate)))
    if n < 0:
        raise ValueError(f"warp_len needs L >= 0 and a rate in [{SPEED_RANGE[0]}, {SPEED_RANGE[1]}], got L = {L}, rate = {rate}")
    return n


PITCH_RANGE = 12.0            # semitones either way: the factors 1/2 .. 2 of Engine.pitch_shift


# ---- option parsing: every "(low, high)", probability and whole number of the samplers and the mixer goes through these
def _pair(name: str, value, low, high, wording: str, form: Optional[str] = "(low, high)", closed: bool = True,
          echo: bool = False, whole: bool = False):
    """The option `name` = (low, high) as two floats with low <= lo <= hi <= high (closed=False: low < lo and hi < high);
    whole=True: exactly two ints (no bool) instead.  What is no such pair is refused as "`name` must be `form`" - with
    form=None by the conversion's own error - and a pair outside the bounds as "`name` must be `wording`", naming the
    value as given or, with echo=True, as parsed."""
    try:
        lo, hi = value if whole else (float(value[0]), float(value[1]))
    except (TypeError, ValueError, IndexError):
        if form is None:
            raise
        raise ValueError(f"{name} must be {form}, got {value}") from None
    ok = not whole or not any(isinstance(v, bool) or not isinstance(v, int) for v in (lo, hi))
    if not (ok and (low <= lo <= hi <= high if closed else low < lo <= hi < high)):
        raise ValueError(f"{name} must be {wording}, got {(lo, hi) if echo else value}")
    return (int(lo), int(hi)) if whole else (lo, hi)


def _positive_pair(name: str, value, form: Optional[str] = "(low, high)"):
    return _pair(name, value, 0.0, math.inf, "(low, high) with 0 < low <= high", form, closed=False)


def _rate_pair(name: str, value):
    lo, hi = SPEED_RANGE
    return _pair(name, value, lo, hi, f"(low, high) with {lo} <= low <= high <= {hi}", "None or (low, high)", echo=True)


def _speed_pair(name: str, value):
    """(low, high) metres per second with 0 <= low <= high < inf."""
    wording = "(low, high) metres per second with 0 <= low <= high"
    lo, hi = _pair(name, value, 0.0, math.inf, wording, "None or (low, high)")
    if hi == math.inf:
        raise ValueError(f"{name} must be {wording}, got {value}")
    return lo, hi


def _probability(name: str, p, as_given: bool = False) -> float:
    if not 0.0 <= (p if as_given else float(p)) <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {p}")
    return float(p)


def _stretch_ranges(tempo=None, pitch=None, speed=None, p_tempo: float = 1.0, p_pitch: float = 1.0, p_speed: float = 1.0):
    """The ranges of the rates DynamicMixer(tempo=, pitch=, speed=) can draw: ((t_lo, t_hi), (p_lo, p_hi), (v_lo, v_hi)),
    with t the tempo, p = 2^(semitones / 12) the pitch factor and v the speed.  An argument that is None gives (1, 1); with
    a probability below 1 the value 1.0 belongs to the range."""
    def widen(r, p):
        return (min(r[0], 1.0), max(r[1], 1.0)) if p < 1.0 else r
    t = widen(tempo, p_tempo) if tempo is not None else (1.0, 1.0)
    f = widen((2.0 ** (pitch[0] / 12.0), 2.0 ** (pitch[1] / 12.0)), p_pitch) if pitch is not None else (1.0, 1.0)
    v = widen(speed, p_speed) if speed is not None else (1.0, 1.0)
    return t, f, v


def stretch_len(L: int, tempo=None, pitch=None, speed=None, p_tempo: float = 1.0, p_pitch: float = 1.0,
                p_speed: float = 1.0) -> int:
    """The batch length DynamicMixer(tempo=, pitch=, speed=, ...) makes of clips of L samples: N1 = warp_len(L, t_hi /
    p_lo) after Engine.stretch, then warp_len(N1, v_hi p_hi) after the one Engine.warp (which runs unless only `tempo`
    is given).  tempo and speed are (low, high) rates, pitch (low, high) in semitones, each or None; with a probability
    below 1 the rate 1.0 counts as part of its range."""
    (_, t_hi), (p_lo, p_hi), (_, v_hi) = _stretch_ranges(tempo, pitch, speed, p_tempo, p_pitch, p_speed)
    n = warp_len(L, t_hi / p_lo)
    return n if pitch is None and speed is None else warp_len(n, v_hi * p_hi)


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
    (int64 [items]) say where item k lies in `data`.  `synthesize` makes the items on the device instead (Engine.noise)."""

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

    draw = None                                   # synthesize: the NoiseDraw the items were made from

    @classmethod
    def synthesize(cls, engine, sampler: "NoiseSampler", items: int, seconds: float, sample_rate: int = 16000,
                   out: Optional[torch.Tensor] = None) -> "NoiseBank":
        """`items` noises of `seconds` each, drawn by `sampler` and made on the device by ONE Engine.noise call (cmgan_noise)
        into a float32 [items, K] allocation that IS the bank's flat `data`: item k starts at k K, nothing is copied.  The
        draw is kept as `draw`.  `out`: a contiguous float32 [items, K] tensor to write instead of a new one."""
        if not isinstance(sampler, NoiseSampler):
            raise TypeError(f"sampler must be a NoiseSampler, got {type(sampler).__name__}")
        if not _whole_in(items, 1, 65535):
            raise ValueError(f"items must be a whole number in [1, 65535], got {items}")
        K = int(round(float(seconds) * sample_rate))
        if K < 1:
            raise ValueError(f"seconds must give at least one sample, got {seconds} s at {sample_rate} Hz")
        return cls._synthesize(engine, sampler, int(items), K, sample_rate, out)

    @classmethod
    def _synthesize(cls, engine, sampler: "NoiseSampler", items: int, K: int, sample_rate: int, out: Optional[torch.Tensor]):
        """`synthesize` for items of K samples."""
        if out is not None and not (isinstance(out, torch.Tensor) and tuple(out.shape) == (items, K) and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{items}, {K}] tensor")
        d = sampler.draw(items, K, sample_rate, device=engine.device)
        rows = engine.noise(d.seed, d.fir, K, env=d.env, env_hop=sampler.hop(sample_rate), tones=d.tones, n_tones=d.n_tones,
                            impulse=d.impulse, out=out)
        index = torch.arange(items, dtype=torch.int64).to(engine.device, non_blocking=True)
        bank = cls(rows.reshape(-1), index * K, torch.full_like(index, K))
        bank.draw = d
        return bank


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


def octave_filterbank(fs, n_bands: int = 7, n_taps: int = 511, f0: float = 125.0) -> torch.Tensor:
    """The FIR filterbank of Engine.rir_bands: float64 [n_bands, n_taps] on the host, n_taps odd, D = (n_taps - 1) / 2.

    Band i is centred at f0 2^i.  On u = log2(f / f0) it has the gain 0.5 (1 + cos(pi (u - i))) for |u - i| < 1, the lowest
    band flat down to DC and the highest flat up to Nyquist, so neighbouring bands sum to one.  The gains are sampled on M
    points, M the smallest power of two >= 8 n_taps; the zero-phase inverse real FFT is centred at D, cut to n_taps taps
    and multiplied by 0.5 (1 - cos(2 pi (j + 1) / (n_taps + 1))).  The last band is then replaced by delta_D minus the sum
    of the others: the bank sums to a pure delay of D samples by construction (n_bands = 1 is delta).  A bank whose
    second-highest centre is not below fs / 2 is rejected."""
    if isinstance(n_bands, bool) or int(n_bands) != n_bands or not 1 <= n_bands <= 8:
        raise ValueError(f"n_bands must be a whole number in [1, 8], got {n_bands}")
    if isinstance(n_taps, bool) or int(n_taps) != n_taps or not 1 <= n_taps <= 1023 or int(n_taps) % 2 != 1:
        raise ValueError(f"n_taps must be an odd whole number in [1, 1023], got {n_taps}")
    fs, f0, NB, NF = float(fs), float(f0), int(n_bands), int(n_taps)
    if not (0.0 < fs < math.inf and 0.0 < f0 < math.inf):
        raise ValueError(f"fs and f0 must be positive and finite, got fs = {fs}, f0 = {f0}")
    if NB >= 2 and not f0 * 2.0 ** (NB - 2) < 0.5 * fs:
        raise ValueError(f"{NB} octave bands from {f0} Hz need the centre {f0 * 2.0 ** (NB - 2)} Hz of the second-highest band "
                         f"below fs / 2 = {0.5 * fs} Hz")
    D = (NF - 1) // 2
    M = 1 << max(0, math.ceil(math.log2(8 * NF)))
    f = np.arange(M // 2 + 1, dtype=np.float64) * (fs / M)
    with np.errstate(divide="ignore"):
        u = np.log2(f / f0)                                          # (-inf at DC: the lowest band's flat side)
    bank = np.zeros((NB, NF))
    j = np.arange(NF)
    window = 0.5 * (1.0 - np.cos(2.0 * np.pi * (j + 1) / (NF + 1)))
    for i in range(NB - 1):
        x = np.clip(u - i, -1.0, 1.0)
        gain = 0.5 * (1.0 + np.cos(np.pi * x))
        if i == 0:
            gain = np.where(u <= 0.0, 1.0, gain)
        bank[i] = np.fft.irfft(gain, M)[(j - D) % M] * window
    bank[NB - 1] = -bank[:NB - 1].sum(axis=0)
    bank[NB - 1, D] += 1.0
    return torch.from_numpy(bank)


def _band_ranges(name: str, value, n: int):
    """`n` (low, high) pairs with 0 <= low <= high < inf."""
    try:
        pairs = tuple((float(lo), float(hi)) for lo, hi in value)
    except (TypeError, ValueError):
        pairs = ()
    if len(pairs) != n or not all(0.0 <= lo <= hi < math.inf for lo, hi in pairs):
        raise ValueError(f"{name} must be None or {n} (low, high) pairs, one per band, with 0 <= low <= high, got {value}")
    return pairs


class TailDraw(NamedTuple):
    """RoomSampler.draw_tail: what Engine.rir_tail needs beyond the responses `draw` was simulated to.  n_full int32 [R],
    the responses' whole lengths; decay float64 [R, max(bands, 1)], the 60 dB decay time per band; seed int64 [R]; with
    `sources` also src_junction int32 [R, n], every located source's own junction, and src_seed int64 [R, n] (a source uses
    its room's n_full and decay)."""
    n_full: torch.Tensor
    decay: torch.Tensor
    seed: torch.Tensor
    src_junction: Optional[torch.Tensor] = None
    src_seed: Optional[torch.Tensor] = None


class RoomSampler:
    """Random shoe-box rooms for Engine.rir: `draw(R, K, fs)` -> `(rooms float64 [R, 15], n_taps int32 [R])`.

    Per row: the size uniform per axis between `dims` = (low, high) (metres), source and receiver uniform and independent
    in the room shrunk by `margin` on every side, rt60 uniform in `rt60` = (low, high) seconds; the six reflection
    coefficients are `sabine_beta(rt60, size)` and n_taps = min(K, ceil(rt60 fs)).  Everything is drawn from `generator`
    (None: the device's default one) on the device with tensor arithmetic: no host synchronisation.

    `bands` = n (1 .. 8) turns on the band model of Engine.rir_bands: walls whose absorption depends on frequency, and air
    absorption, in n octave bands from 125 Hz joined by `octave_filterbank(fs, n, filter_taps)`.  `draw_bands(rooms)`,
    called after `draw`, gives the float64 [R, n, 7] band table.  `tilt` = (low, high) is drawn per room, in octaves of
    absorption growth per octave of frequency: alpha_b = clamp(alpha 2^(tilt (b - b_ref)), 0, 1) with alpha = 1 - beta^2 of
    the table and b_ref the band nearest 1 kHz, so by Sabine's formula band b has the reverberation time rt60 2^(-tilt (b -
    b_ref)) while its alpha_b stays below 1, and at 1 kHz the room is the one `draw` made.  `air` is None (no air
    absorption) or n (low, high) ranges of the amplitude attenuation m_b in nepers per metre, drawn per room; there is no
    default table of a "standard atmosphere": the values are the caller's.  Without `bands` (the default) the sampler is
    what it was: the same draws from the generator, and `draw_bands` is an error.

    `tail_ms` = a float turns on the hybrid of Engine.rir_tail: the image-source method only up to a JUNCTION `tail_ms`
    milliseconds after the direct sound, a diffuse tail of decaying noise from there on.  `draw` then returns as n_taps the
    junction min(n_full, ceil((|source - receiver| / c + tail_ms / 1000) fs)), n_full the n_taps above, and `n_images`
    covers only the largest junction the sampler can draw - that is where the saving comes from.  `draw_tail(rooms, fs)`,
    called after `draw` (and `draw_bands`, and `draw_sources`), gives a TailDraw: n_full, the decay times - the drawn rt60
    itself, or with `bands` 1 / decay_b = 1 / (rt60 2^(-tilt (b - b_ref))) + m_b c / (3 ln 10), walls and air, from the rt60
    and tilt that were drawn and not from the table's coefficients - and int64 noise seeds, a torch.randint from
    `generator` on the device after every other draw.  The tail's level is fitted to the `tail_window_ms` in front of the
    junction, so tail_ms must exceed that window (with `bands`, by the filterbank's delay too).  With None (the default)
    the sampler draws the same numbers as before and `draw_tail` is an error.

    `source_pattern` / `mic_pattern` = (low, high) in [0, 1] turn on directivity (Engine.rir(orient=, pattern=)): a
    first-order pattern alpha + (1 - alpha) cos(theta) at the talker and at the microphone, alpha uniform per row in its
    range (1 omni, 0.5 cardioid, 0 figure-of-eight; None: 1).  `draw_dirs(tables)`, called after every other draw, gives
    (orient float64 [..., 6], pattern float64 [..., max(bands, 1), 2]) for the [R, 15] table of `draw`, the [R, n, 15] of
    `draw_sources` or, with path=True, the [..., P, 15] of `draw_path`: the talker's facing vector u at an angle uniform
    in `facing_deg` = (low, high) degrees off the direction from source to receiver (0: facing the microphone) and an
    azimuth uniform around it, the microphone's vector v uniform on the sphere.  With `bands`, alpha_s,b = clamp(alpha_s -
    tilt (b - b_ref), 0, 1) with tilt drawn per row in `pattern_tilt` (per octave: more directional upwards); alpha_m
    is flat.  On a path every waypoint keeps the row's angle, azimuth and patterns around ITS OWN direction to the
    receiver: the talker keeps half-facing the microphone as it walks.  With all four at their defaults the sampler draws
    what it drew before and `draw_dirs` is an error."""

    BAND_F0 = 125.0               # Hz: the centre of band 0

    def __init__(self, dims=((3.0, 3.0, 2.5), (10.0, 8.0, 4.0)), rt60=(0.2, 0.8), margin: float = 0.5,
                 generator: Optional[torch.Generator] = None, bands: Optional[int] = None, tilt=(0.0, 0.0), air=None,
                 filter_taps: int = 511, tail_ms: Optional[float] = None, tail_window_ms: float = 30.0,
                 source_pattern=None, facing_deg=(0.0, 180.0), mic_pattern=None, pattern_tilt=(0.0, 0.0)):
        try:
            lo, hi = (tuple(float(v) for v in d) for d in dims)
        except (TypeError, ValueError):
            raise ValueError(f"dims must be ((Lx, Ly, Lz) low, (Lx, Ly, Lz) high), got {dims}") from None
        if len(lo) != 3 or len(hi) != 3 or not all(0.0 < a <= b < math.inf for a, b in zip(lo, hi)):
            raise ValueError(f"dims must be ((Lx, Ly, Lz) low, (Lx, Ly, Lz) high) with 0 < low <= high, got {dims}")
        t_lo, t_hi = _positive_pair("rt60", rt60, form=None)
        margin = float(margin)
        if not 0.0 <= margin < 0.5 * min(lo):
            raise ValueError(f"margin must lie in [0, {0.5 * min(lo)}): half the smallest room size of {dims}, got {margin}")
        self.lo, self.hi, self.rt60, self.margin, self.generator = lo, hi, (t_lo, t_hi), margin, generator
        if bands is None:
            if tuple(tilt) != (0.0, 0.0) or air is not None:
                raise ValueError("tilt and air belong to the band model: give bands=n with them")
            self.bands, self.tilt, self.air, self.filter_taps, self.band_ref = None, (0.0, 0.0), None, int(filter_taps), 0
        else:
            if isinstance(bands, bool) or int(bands) != bands or not 1 <= bands <= 8:
                raise ValueError(f"bands must be None or a band count in [1, 8], got {bands}")
            if isinstance(filter_taps, bool) or int(filter_taps) != filter_taps or not 1 <= filter_taps <= 1023 \
                    or int(filter_taps) % 2 != 1:
                raise ValueError(f"filter_taps must be an odd whole number in [1, 1023], got {filter_taps}")
            self.bands, self.filter_taps = int(bands), int(filter_taps)
            self.tilt = _pair("tilt", tilt, -math.inf, math.inf, "(low, high) with finite low <= high", closed=False, echo=True)
            self.air = None if air is None else _band_ranges("air", air, self.bands)
            # the band nearest 1 kHz on the octave scale
            self.band_ref = min(max(int(round(math.log2(1000.0 / self.BAND_F0))), 0), self.bands - 1)
        self._filters = {}
        if tail_ms is not None:
            if isinstance(tail_ms, bool) or not isinstance(tail_ms, (int, float)) or not 0.0 < tail_ms < math.inf:
                raise ValueError(f"tail_ms must be None or a positive, finite number of milliseconds, got {tail_ms}")
            tail_ms = float(tail_ms)
        if isinstance(tail_window_ms, bool) or not isinstance(tail_window_ms, (int, float)) or not 0.0 < tail_window_ms < math.inf:
            raise ValueError(f"tail_window_ms must be a positive, finite number of milliseconds, got {tail_window_ms}")
        self.tail_ms, self.tail_window_ms = tail_ms, float(tail_window_ms)
        self._drawn = {}              # tail_ms: the rt60, n_full (draw), tilt and m (draw_bands) of the last draw, for draw_tail
        # ---- directivity: judged last, so that every earlier error is what it was
        self.directional = source_pattern is not None or mic_pattern is not None
        alphas = lambda name, v: None if v is None else _pair(name, v, 0.0, 1.0, "None or (low, high) with 0 <= low <= high <= 1",
                                                              "None or (low, high)", echo=True)
        self.source_pattern, self.mic_pattern = alphas("source_pattern", source_pattern), alphas("mic_pattern", mic_pattern)
        self.facing_deg = _pair("facing_deg", facing_deg, 0.0, 180.0, "(low, high) degrees with 0 <= low <= high <= 180", echo=True)
        self.pattern_tilt = _pair("pattern_tilt", pattern_tilt, -math.inf, math.inf, "(low, high) with finite low <= high",
                                  closed=False, echo=True)
        if not self.directional and (self.facing_deg != (0.0, 180.0) or self.pattern_tilt != (0.0, 0.0)):
            raise ValueError("facing_deg and pattern_tilt belong to directivity: give source_pattern or mic_pattern with them")
        if self.pattern_tilt != (0.0, 0.0) and (self.bands is None or self.source_pattern is None):
            raise ValueError("pattern_tilt tilts the talker's pattern over the bands: give bands=n and source_pattern with it")

    def max_junction(self, K: int, fs: int, c: float = SPEED_OF_SOUND) -> int:
        """The largest n_taps `draw` can return: K, or with `tail_ms` min(K, ceil((d / c + tail_ms / 1000) fs)) with d the
        diagonal of the UPPER size bound shrunk by the margin, the farthest a source can be from a receiver."""
        if self.tail_ms is None:
            return K
        d = math.sqrt(sum((l - 2.0 * self.margin) ** 2 for l in self.hi))
        return min(K, int(math.ceil((d / c + self.tail_ms / 1000.0) * fs)))

    def n_images(self, K: int, fs: int, c: float = SPEED_OF_SOUND, tw: int = RIR_TW):
        """(Nx, Ny, Nz) that leaves out no image of a K-tap response in any room this sampler draws: host arithmetic on
        the LOWER size bound, ceil((K + tw) c / fs / (2 Lmin_axis)) + 1.  With `bands` the ranges cover K + D taps, D the
        filterbank's delay: Engine.rir_bands simulates the bands that far.  With `tail_ms` K is `max_junction(K, fs)`:
        the images stop at the junction."""
        K = self.max_junction(K, fs, c)
        if self.bands is not None:
            K = K + (self.filter_taps - 1) // 2
        return tuple(int(math.ceil((K + tw) * c / fs / (2.0 * l))) + 1 for l in self.lo)

    def filters(self, fs: int, device=None) -> torch.Tensor:
        """`octave_filterbank(fs, bands, filter_taps)` on `device`: computed once per (fs, device) and kept."""
        if self.bands is None:
            raise ValueError("this RoomSampler has no bands")
        key = (int(fs), str(device))
        if key not in self._filters:
            self._filters[key] = octave_filterbank(fs, self.bands, self.filter_taps, self.BAND_F0).to(device or "cpu")
        return self._filters[key]

    def draw_bands(self, rooms: torch.Tensor) -> torch.Tensor:
        """The band table of rooms that `draw` made: float64 [R, bands, 7] for a drawn [R, 15] one, per band the six
        reflection coefficients and m.  One rand(R, 1 + bands) from `generator` on the device of `rooms`, after the
        room draws: column 0 is the room's tilt, column 1 + b the place of m_b in its range.  Per wall beta_b =
        sqrt(1 - alpha_b); a band whose factor 2^(tilt (b - b_ref)) is exactly 1 keeps the table's beta itself."""
        if self.bands is None:
            raise ValueError("this RoomSampler has no bands")
        if not isinstance(rooms, torch.Tensor) or rooms.dtype != torch.float64 or rooms.dim() != 2 or rooms.size(1) != 15:
            raise ValueError("rooms must be a float64 [R, 15] table of RoomSampler.draw")
        R, n = rooms.size(0), self.bands
        u = torch.rand(R, 1 + n, dtype=torch.float64, generator=self.generator, device=rooms.device)
        tilt = self.tilt[0] + (self.tilt[1] - self.tilt[0]) * u[:, 0]
        step = torch.arange(n, dtype=torch.float64).to(rooms.device, non_blocking=True) - float(self.band_ref)
        octaves = tilt[:, None] * step[None, :]                                        # [R, n]
        beta = rooms[:, None, 9:15]                                                   # [R, 1, 6]
        alpha = ((1.0 - beta * beta) * torch.exp2(octaves)[:, :, None]).clamp(0.0, 1.0)
        walls = torch.where((octaves == 0.0)[:, :, None], beta.expand(R, n, 6), torch.sqrt(1.0 - alpha))
        if self.air is None:
            m = torch.zeros(R, n, dtype=torch.float64, device=rooms.device)
        else:
            lo = torch.tensor([p[0] for p in self.air], dtype=torch.float64).to(rooms.device, non_blocking=True)
            hi = torch.tensor([p[1] for p in self.air], dtype=torch.float64).to(rooms.device, non_blocking=True)
            m = lo + (hi - lo) * u[:, 1:]
        if self.tail_ms is not None:
            self._drawn.update(tilt=tilt, m=m)
        return torch.cat([walls, m[:, :, None]], dim=2).contiguous()

    def _junction(self, tables: torch.Tensor, n_full: torch.Tensor, fs: int) -> torch.Tensor:
        """min(n_full, ceil((|source - receiver| / c + tail_ms / 1000) fs)) of [..., 15] tables, int32."""
        direct = torch.linalg.vector_norm(tables[..., 3:6] - tables[..., 6:9], dim=-1) / SPEED_OF_SOUND
        return torch.minimum(torch.ceil((direct + self.tail_ms / 1000.0) * fs).to(torch.int32), n_full)

    def draw_tail(self, rooms: torch.Tensor, fs: int, sources: Optional[torch.Tensor] = None) -> TailDraw:
        """The TailDraw of rooms that `draw` made last (and `draw_bands`, with bands; `sources`: the [R, n, 15] tables of
        `draw_sources`).  Only the seeds are drawn: torch.randint(R) and, with sources, torch.randint(R, n) from
        `generator` on the device of `rooms`; the rest is arithmetic on what the earlier draws kept."""
        if self.tail_ms is None:
            raise ValueError("this RoomSampler has no tail_ms")
        if not isinstance(rooms, torch.Tensor) or rooms.dtype != torch.float64 or rooms.dim() != 2 or rooms.size(1) != 15:
            raise ValueError("rooms must be a float64 [R, 15] table of RoomSampler.draw")
        R, kept = rooms.size(0), self._drawn
        need = ("rt", "n_full") if self.bands is None else ("rt", "n_full", "tilt", "m")
        if any(k not in kept or kept[k].size(0) != R or kept[k].device != rooms.device for k in need):
            raise ValueError("draw_tail follows draw (and draw_bands, with bands) of the same rooms")
        W = int(self.tail_window_ms * float(fs) / 1000.0 + 0.5)
        D = 0 if self.bands is None else (self.filter_taps - 1) // 2
        if not 1 <= W <= RIR_TAIL_MAX_WINDOW or math.ceil(self.tail_ms / 1000.0 * fs) < W + D:
            raise ValueError(f"tail_ms = {self.tail_ms} at fs = {fs} must leave room for the fit window of tail_window_ms = "
                             f"{self.tail_window_ms} (1 .. {RIR_TAIL_MAX_WINDOW} samples) and the filterbank's delay of {D} samples")
        rt = kept["rt"]
        if self.bands is None:
            decay = rt[:, None].contiguous()
        else:
            step = torch.arange(self.bands, dtype=torch.float64).to(rooms.device, non_blocking=True) - float(self.band_ref)
            walls = rt[:, None] * torch.exp2(-kept["tilt"][:, None] * step[None, :])
            decay = (1.0 / (1.0 / walls + kept["m"] * (SPEED_OF_SOUND / THREE_LN10))).contiguous()
        draw = lambda *shape: torch.randint(0, 2 ** 63 - 1, shape, dtype=torch.int64, generator=self.generator,
                                            device=rooms.device)
        seed = draw(R)
        if sources is None:
            return TailDraw(kept["n_full"], decay, seed)
        if not isinstance(sources, torch.Tensor) or sources.dtype != torch.float64 or sources.dim() != 3 \
                or sources.size(0) != R or sources.size(2) != 15:
            raise ValueError(f"sources must be the float64 [{R}, n, 15] tables of RoomSampler.draw_sources")
        junction = self._junction(sources, kept["n_full"][:, None], fs).contiguous()
        return TailDraw(kept["n_full"], decay, seed, junction, draw(R, sources.size(1)))

    def draw_dirs(self, tables: torch.Tensor, path: bool = False, facing_deg=None):
        """(orient float64 [..., 6], pattern float64 [..., max(bands, 1), 2]) for [..., 15] tables this sampler drew: the
        tables of Engine.rir(orient=, pattern=) / Engine.rir_bands after a reshape to rows.  ONE rand(..., 7) from
        `generator` on the device of `tables`, after every other draw: the places of alpha_s, alpha_m, the facing angle,
        its azimuth, v's height and azimuth, and the tilt.  path=True: `tables` is [..., P, 15] of `draw_path`, drawn once
        per walk (rand(..., 7) without the P) and applied at every waypoint.  `facing_deg` overrides the sampler's range
        (DynamicMixer gives further sources (0, 180))."""
        if not self.directional:
            raise ValueError("this RoomSampler has no source_pattern or mic_pattern")
        need = (3, 4) if path else (2, 3)
        if not isinstance(tables, torch.Tensor) or tables.dtype != torch.float64 or tables.dim() not in need or tables.size(-1) != 15:
            raise ValueError("tables must be the float64 [R, 15] table of RoomSampler.draw, the [R, n, 15] ones of draw_sources "
                             "or, with path=True, the [..., P, 15] ones of draw_path")
        f_lo, f_hi = self.facing_deg if facing_deg is None else _pair(
            "facing_deg", facing_deg, 0.0, 180.0, "(low, high) degrees with 0 <= low <= high <= 180", echo=True)
        dev, nb = tables.device, self.bands or 1
        lead = tuple(tables.shape[:-2] if path else tables.shape[:-1])
        u = torch.rand(*lead, 7, dtype=torch.float64, generator=self.generator, device=dev)
        if path:
            u = u[..., None, :]                                   # one draw per walk, at every waypoint
        between = lambda rng, x: torch.ones_like(x) if rng is None else rng[0] + (rng[1] - rng[0]) * x
        alpha_s, alpha_m = between(self.source_pattern, u[..., 0]), between(self.mic_pattern, u[..., 1])
        theta = torch.deg2rad(between((f_lo, f_hi), u[..., 2]))[..., None]
        phi = (2.0 * math.pi) * u[..., 3:4]
        # the cone around w, the direction from source to receiver (the x axis where the two coincide)
        w = tables[..., 6:9] - tables[..., 3:6]
        far = torch.linalg.vector_norm(w, dim=-1, keepdim=True)
        ex = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).to(dev, non_blocking=True)
        ey = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).to(dev, non_blocking=True)
        w = torch.where(far > 0.0, w / torch.where(far > 0.0, far, torch.ones_like(far)), ex)
        e1 = torch.linalg.cross(w, torch.where(w[..., 0:1].abs() < 0.9, ex, ey).expand_as(w), dim=-1)
        e1 = e1 / torch.linalg.vector_norm(e1, dim=-1, keepdim=True)
        e2 = torch.linalg.cross(w, e1, dim=-1)
        facing = torch.cos(theta) * w + torch.sin(theta) * (torch.cos(phi) * e1 + torch.sin(phi) * e2)
        z = 2.0 * u[..., 4:5] - 1.0                               # v uniform on the sphere: height uniform, then the azimuth
        rho, psi = torch.sqrt((1.0 - z * z).clamp_min(0.0)), (2.0 * math.pi) * u[..., 5:6]
        mic = torch.cat([rho * torch.cos(psi), rho * torch.sin(psi), z], dim=-1).expand_as(facing)
        step = torch.arange(nb, dtype=torch.float64).to(dev, non_blocking=True) - float(self.band_ref)
        tilt = between(self.pattern_tilt, u[..., 6])
        per_band = (alpha_s[..., None] - tilt[..., None] * step).clamp(0.0, 1.0)              # [..., nb]
        pattern = torch.stack([per_band, alpha_m[..., None].expand_as(per_band)], dim=-1)
        if path:
            pattern = pattern.expand(*tables.shape[:-1], nb, 2)
        return torch.cat([facing, mic], dim=-1).contiguous(), pattern.contiguous()

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
        if self.tail_ms is not None:
            self._drawn = dict(rt=rt, n_full=n_taps)
            n_taps = self._junction(rooms, n_taps, fs)
        return rooms, n_taps

    def draw_sources(self, rooms: torch.Tensor, n: int) -> torch.Tensor:
        """Further source positions in rooms that `draw` made: float64 [R, n, 15] tables for a drawn [R, 15] one.  Row
        (r, j) keeps room r's size, receiver and reflection coefficients; its source is uniform in the room shrunk by
        `margin`, independent of the room's own, drawn from `generator` on the device of `rooms` (so: after the room
        draws).  `tables.reshape(R * n, 15)` with each room's n_taps repeated n times is one Engine.rir call."""
        if not isinstance(rooms, torch.Tensor) or rooms.dtype != torch.float64 or rooms.dim() != 2 or rooms.size(1) != 15:
            raise ValueError("rooms must be a float64 [R, 15] table of RoomSampler.draw")
        if isinstance(n, bool) or int(n) != n or n < 1:
            raise ValueError(f"n must be a source count >= 1, got {n}")
        R, n = rooms.size(0), int(n)
        u = torch.rand(R, n, 3, dtype=torch.float64, generator=self.generator, device=rooms.device)
        inner = rooms[:, None, 0:3] - 2.0 * self.margin
        out = rooms[:, None, :].expand(R, n, 15).clone()
        out[:, :, 3:6] = self.margin + inner * u
        return out

    def draw_path(self, rooms: torch.Tensor, P: int, seconds: float, speed=(0.5, 1.5)) -> torch.Tensor:
        """A straight walk per source for Engine.scene_path: float64 [R, P, 15] tables for the [R, 15] one `draw` made, or
        [R, n, P, 15] for the [R, n, 15] ones of `draw_sources`.  Every waypoint keeps the room's size, receiver and
        reflection coefficients.  Waypoint 0 is the drawn source position; an end point is drawn uniform in the room
        shrunk by `margin` and a speed uniform in `speed` = (low, high) metres per second; a segment longer than
        speed x `seconds` is shortened to that (the room is convex, so it stays inside), and the P waypoints are spaced
        linearly on it, `seconds` apart from first to last.  ONE rand(R, 4) (rand(R, n, 4)) from `generator` on the device
        of `rooms`: the end point, then the speed - so: after every other draw of the sampler.
        `tables.reshape(-1, 15)` with each room's n_taps repeated is one Engine.rir / Engine.rir_bands call."""
        if not isinstance(rooms, torch.Tensor) or rooms.dtype != torch.float64 or rooms.dim() not in (2, 3) or rooms.size(-1) != 15:
            raise ValueError("rooms must be a float64 [R, 15] table of RoomSampler.draw or the [R, n, 15] ones of draw_sources")
        if not _whole_in(P, 1, SCENE_MAX_WAYPOINTS):
            raise ValueError(f"P must be a waypoint count in [1, {SCENE_MAX_WAYPOINTS}], got {P}")
        if isinstance(seconds, bool) or not isinstance(seconds, (int, float)) or not 0.0 < seconds < math.inf:
            raise ValueError(f"seconds must be positive and finite, got {seconds}")
        lo, hi = _speed_pair("speed", speed)
        P, lead = int(P), tuple(rooms.shape[:-1])
        u = torch.rand(*lead, 4, dtype=torch.float64, generator=self.generator, device=rooms.device)
        start = rooms[..., 3:6]
        step = self.margin + (rooms[..., 0:3] - 2.0 * self.margin) * u[..., 0:3] - start
        far = torch.linalg.vector_norm(step, dim=-1, keepdim=True)
        reach = (lo + (hi - lo) * u[..., 3:4]) * float(seconds)
        step = step * torch.where(far > reach, reach / torch.where(far > reach, far, torch.ones_like(far)), torch.ones_like(far))
        along = torch.arange(P, dtype=torch.float64).to(rooms.device, non_blocking=True) / float(max(P - 1, 1))
        out = rooms[..., None, :].expand(*lead, P, 15).clone()
        out[..., 3:6] = start[..., None, :] + step[..., None, :] * along[:, None]
        return out


# ---- biquad designs: R. Bristow-Johnson's audio-EQ-cookbook formulas, normalised to a0 = 1 --------------------------
def _f64(v, like=None) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.to(torch.float64)
    return torch.as_tensor(v, dtype=torch.float64, device=like.device if isinstance(like, torch.Tensor) else None)


def _cookbook(f0, q, fs):
    f0 = _f64(f0)
    q = _f64(q, f0)
    w0 = 2.0 * math.pi * f0 / fs
    return torch.cos(w0), torch.sin(w0) / (2.0 * q)


def _sos_rows(b0, b1, b2, a0, a1, a2) -> torch.Tensor:
    """[..., 6] rows in scipy's layout (b0 b1 b2 a0 a1 a2), divided by a0 so that a0 is exactly 1."""
    b0, b1, b2, a0, a1, a2 = torch.broadcast_tensors(b0, b1, b2, a0, a1, a2)
    return torch.stack([b0 / a0, b1 / a0, b2 / a0, torch.ones_like(a0), a1 / a0, a2 / a0], dim=-1)


def biquad_peaking(f0, gain_db, q, fs) -> torch.Tensor:
    """A peaking-EQ section: gain_db at f0 (Hz), bandwidth set by q, unity far from f0.  Plain float64 tensor arithmetic on
    the device of its arguments (like every design here); returns [..., 6] rows for Engine.channel."""
    cw, alpha = _cookbook(f0, q, fs)
    A = torch.pow(10.0, _f64(gain_db, cw) / 40.0)
    return _sos_rows(1.0 + alpha * A, -2.0 * cw, 1.0 - alpha * A, 1.0 + alpha / A, -2.0 * cw, 1.0 - alpha / A)


def biquad_low_shelf(f0, gain_db, q, fs) -> torch.Tensor:
    """A low-shelf section: gain_db at DC, unity at Nyquist, the midpoint (gain_db / 2) at f0."""
    cw, alpha = _cookbook(f0, q, fs)
    A = torch.pow(10.0, _f64(gain_db, cw) / 40.0)
    r = 2.0 * torch.sqrt(A) * alpha
    return _sos_rows(A * ((A + 1.0) - (A - 1.0) * cw + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cw),
                     A * ((A + 1.0) - (A - 1.0) * cw - r), (A + 1.0) + (A - 1.0) * cw + r,
                     -2.0 * ((A - 1.0) + (A + 1.0) * cw), (A + 1.0) + (A - 1.0) * cw - r)


def biquad_high_shelf(f0, gain_db, q, fs) -> torch.Tensor:
    """A high-shelf section: gain_db at Nyquist, unity at DC, the midpoint (gain_db / 2) at f0."""
    cw, alpha = _cookbook(f0, q, fs)
    A = torch.pow(10.0, _f64(gain_db, cw) / 40.0)
    r = 2.0 * torch.sqrt(A) * alpha
    return _sos_rows(A * ((A + 1.0) + (A - 1.0) * cw + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cw),
                     A * ((A + 1.0) + (A - 1.0) * cw - r), (A + 1.0) - (A - 1.0) * cw + r,
                     2.0 * ((A - 1.0) - (A + 1.0) * cw), (A + 1.0) - (A - 1.0) * cw - r)


def biquad_lowpass(f0, q, fs) -> torch.Tensor:
    """A 2nd-order low-pass with corner f0: unity at DC, |H(f0)| = q (q = 1 / sqrt(2): Butterworth, -3.01 dB at f0)."""
    cw, alpha = _cookbook(f0, q, fs)
    return _sos_rows(0.5 * (1.0 - cw), 1.0 - cw, 0.5 * (1.0 - cw), 1.0 + alpha, -2.0 * cw, 1.0 - alpha)


def biquad_highpass(f0, q, fs) -> torch.Tensor:
    """A 2nd-order high-pass with corner f0: unity at Nyquist, |H(f0)| = q."""
    cw, alpha = _cookbook(f0, q, fs)
    return _sos_rows(0.5 * (1.0 + cw), -(1.0 + cw), 0.5 * (1.0 + cw), 1.0 + alpha, -2.0 * cw, 1.0 - alpha)


def butter_lowpass_sos(order: int, fc, fs) -> torch.Tensor:
    """An even-order (2 .. 8) Butterworth low-pass at fc as [..., order / 2, 6]: the cascade of cookbook low-passes with
    Q_k = 1 / (2 cos(pi (2k + 1) / (2 order))), which has the frequency response of scipy.signal.butter's design."""
    if isinstance(order, bool) or int(order) != order or order not in (2, 4, 6, 8):
        raise ValueError(f"order must be 2, 4, 6 or 8, got {order}")
    fc = _f64(fc)
    return torch.stack([biquad_lowpass(fc, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (2 * order))), fs)
                        for k in range(order // 2)], dim=-2)


class ChannelSampler:
    """Random recording channels for Engine.channel: `draw(B, fs, device)` -> `(sos float64 [B, S, 6], n_sections int32
    [B], n_shared int32 [B], clip_rel float64 [B])`.

    Per row, in this order of the cascade: with probability `p_highpass` a 2nd-order Butterworth high-pass, corner
    log-uniform in `highpass_hz`; 0 .. `max_eq` (uniform) equaliser sections, each a peaking section, a low shelf or a high
    shelf with equal probability, f0 log-uniform in `eq_hz` (None: 50 Hz .. 0.45 fs), gain uniform in +-`eq_db`, Q
    uniform in `eq_q`; with probability `p_bandlimit` a Butterworth low-pass of `bandlimit_order` (even, 2 .. 8), cutoff
    uniform in `bandlimit_hz`; with probability `p_clip` a clipping level as a fraction of the row's peak, uniform in
    `clip_rel` (+inf for the other rows).  S = [p_highpass > 0] + max_eq + [p_bandlimit > 0] bandlimit_order / 2 (at least
    1) is fixed by the options and may not exceed 8; a row's sections are packed to the front, the rest are the identity
    (1 0 0 1 0 0).  n_shared says how many of a row's leading sections DynamicMixer(channel_on="both") also applies to the
    target: all of them (the clip is the noisy signal's alone).  Everything is drawn from `generator` (None: the
    device's default one) on the device with tensor arithmetic: no host synchronisation.  Every cookbook section with
    0 < f0 < fs / 2 and Q > 0 lies inside the stability triangle, so no row of a draw is invalid."""

    def __init__(self, p_highpass: float = 0.5, highpass_hz=(20.0, 120.0), max_eq: int = 3, eq_hz=None, eq_db: float = 6.0,
                 eq_q=(0.5, 2.0), p_bandlimit: float = 0.2, bandlimit_hz=(3400.0, 3800.0), bandlimit_order: int = 8,
                 p_clip: float = 0.1, clip_rel=(0.3, 0.9), generator: Optional[torch.Generator] = None):
        self.p_highpass, self.p_bandlimit, self.p_clip = (
            _probability(name, p) for name, p in (("p_highpass", p_highpass), ("p_bandlimit", p_bandlimit), ("p_clip", p_clip)))
        self.highpass_hz = _positive_pair("highpass_hz", highpass_hz)
        self.eq_hz = None if eq_hz is None else _positive_pair("eq_hz", eq_hz)
        self.eq_q = _positive_pair("eq_q", eq_q)
        self.bandlimit_hz = _positive_pair("bandlimit_hz", bandlimit_hz)
        self.clip_rel = _positive_pair("clip_rel", clip_rel)
        if isinstance(max_eq, bool) or int(max_eq) != max_eq or max_eq < 0:
            raise ValueError(f"max_eq must be a section count >= 0, got {max_eq}")
        eq_db = float(eq_db)
        if not 0.0 <= eq_db < math.inf:
            raise ValueError(f"eq_db must be >= 0 and finite, got {eq_db}")
        if isinstance(bandlimit_order, bool) or bandlimit_order not in (2, 4, 6, 8):
            raise ValueError(f"bandlimit_order must be 2, 4, 6 or 8, got {bandlimit_order}")
        self.max_eq, self.eq_db, self.bandlimit_order, self.generator = int(max_eq), eq_db, int(bandlimit_order), generator
        self.n_hp = 1 if self.p_highpass > 0.0 else 0
        self.n_bl = self.bandlimit_order // 2 if self.p_bandlimit > 0.0 else 0
        total = self.n_hp + self.max_eq + self.n_bl
        if total > 8:
            raise ValueError(f"a high-pass, {self.max_eq} equaliser sections and a band limit of order {bandlimit_order} "
                             f"are {total} sections; Engine.channel takes up to 8")
        self.sections = max(total, 1)

    def draw(self, B: int, fs: int, device=None):
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        fs = float(fs)
        eq_hz = self.eq_hz if self.eq_hz is not None else (50.0, 0.45 * fs)
        for name, (lo, hi) in (("highpass_hz", self.highpass_hz), ("eq_hz", eq_hz), ("bandlimit_hz", self.bandlimit_hz)):
            if not (lo <= hi and hi < 0.5 * fs):
                raise ValueError(f"{name} = {(lo, hi)} must lie below fs / 2 = {0.5 * fs} Hz")
        E = self.max_eq
        u = torch.rand(B, 7 + 4 * E, dtype=torch.float64, generator=gen, device=device)
        log_uniform = lambda r, v: math.log(r[0]) + (math.log(r[1]) - math.log(r[0])) * v
        uniform = lambda r, v: r[0] + (r[1] - r[0]) * v
        rows, use = [], []
        if self.n_hp:
            rows.append(biquad_highpass(torch.exp(log_uniform(self.highpass_hz, u[:, 1])), math.sqrt(0.5), fs)[:, None])
            use.append((u[:, 0] < self.p_highpass)[:, None])
        if E:
            n_eq = torch.clamp((u[:, 2] * (E + 1)).to(torch.int64), max=E)
            v = u[:, 7:].reshape(B, E, 4)
            f0 = torch.exp(log_uniform(eq_hz, v[..., 1]))
            gain = self.eq_db * (2.0 * v[..., 2] - 1.0)
            q = uniform(self.eq_q, v[..., 3])
            kind = torch.clamp((v[..., 0] * 3).to(torch.int64), max=2)[..., None]
            rows.append(torch.where(kind == 0, biquad_peaking(f0, gain, q, fs),
                                    torch.where(kind == 1, biquad_low_shelf(f0, gain, q, fs),
                                                biquad_high_shelf(f0, gain, q, fs))))
            use.append(torch.arange(E, device=device)[None, :] < n_eq[:, None])
        if self.n_bl:
            rows.append(butter_lowpass_sos(self.bandlimit_order, uniform(self.bandlimit_hz, u[:, 4]), fs))
            use.append((u[:, 3] < self.p_bandlimit)[:, None].expand(B, self.n_bl))
        identity = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], dtype=torch.float64).to(device, non_blocking=True)
        if rows:
            sos, use = torch.cat(rows, dim=1), torch.cat(use, dim=1)
            sos = torch.where(use[..., None], sos, identity)
            order = torch.argsort((~use).to(torch.int8), dim=1, stable=True)          # a row's own sections first, in order
            sos = torch.gather(sos, 1, order[..., None].expand(B, sos.size(1), 6)).contiguous()
            n_sections = use.sum(dim=1).to(torch.int32)
        else:
            sos = identity.expand(B, 1, 6).contiguous()
            n_sections = torch.zeros(B, dtype=torch.int32, device=device)
        clip = torch.where(u[:, 5] < self.p_clip, uniform(self.clip_rel, u[:, 6]), torch.full_like(u[:, 6], math.inf))
        return sos, n_sections, n_sections.clone(), clip


# ---- dynamics: the table of Engine.dynamics from ratios and milliseconds, and a sampler of it ------------------------
def dynamics_params(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db, fs) -> torch.Tensor:
    """The float64 [..., 6] table of Engine.dynamics, (thr_db, slope, knee_db, a_att, a_rel, makeup_db) per row: slope =
    1 - 1 / ratio (ratio = inf: 1, a limiter) and a = exp(-1 / (t fs)) for a time constant of t = ms / 1000 seconds (0 ms:
    a = 0, instant).  Plain float64 tensor arithmetic on the device of its arguments, like the biquad designs; what the
    result allows (ratio >= 1, knee >= 0, times >= 0) is judged per row by the kernels."""
    thr = _f64(threshold_db)
    ratio, knee, att, rel, makeup = (_f64(v, thr) for v in (ratio, knee_db, attack_ms, release_ms, makeup_db))
    coeff = lambda ms: torch.exp(-1000.0 / (ms * float(fs)))
    thr, slope, knee, a_att, a_rel, makeup = torch.broadcast_tensors(thr, 1.0 - 1.0 / ratio, knee, coeff(att), coeff(rel), makeup)
    return torch.stack([thr, slope, knee, a_att, a_rel, makeup], dim=-1).contiguous()


class DynamicsSampler:
    """Random gain controls for Engine.dynamics: `draw(B, fs, device)` -> a float64 [B, 6] table (threshold_rel_db, slope,
    knee_db, a_att, a_rel, m), and `table(drawn, wav)` -> the float64 [B, 6] table of Engine.dynamics for a batch.

    Per row, with probability `p`, a processor: the threshold uniform in `threshold_rel_db`, in dB RELATIVE to the row's
    peak where the processor runs (as ChannelSampler's clip_rel is); the ratio log-uniform in `ratio`, or infinite - a
    limiter - with probability `p_limiter`; the knee width uniform in `knee_db`; attack and release times log-uniform in
    `attack_ms` and `release_ms`; and m uniform in `makeup`, the share of the reduction at the row's peak that the
    make-up gain gives back: makeup_db = m slope max(0, peak_db - thr_db).  A row that is not chosen gets slope 0 and m 0,
    so Engine.dynamics copies it bit for bit.  `table` fills in the peak: thr_db = 20 log10(max |wav|) + threshold_rel_db;
    a row that is silent or holds a non-finite sample gets slope 0 and make-up 0 as well.  Everything is drawn from
    `generator` (None: the device's default one) on the device with tensor arithmetic: no host synchronisation."""

    def __init__(self, p: float = 0.5, threshold_rel_db=(-30.0, -6.0), ratio=(2.0, 20.0), p_limiter: float = 0.2,
                 knee_db=(0.0, 12.0), attack_ms=(1.0, 30.0), release_ms=(50.0, 500.0), makeup=(0.0, 1.0),
                 generator: Optional[torch.Generator] = None):
        self.p, self.p_limiter = _probability("p", p), _probability("p_limiter", p_limiter)
        self.threshold_rel_db = _pair("threshold_rel_db", threshold_rel_db, -math.inf, math.inf, "(low, high) with finite low <= high",
                                      closed=False)
        self.ratio = _pair("ratio", ratio, 1.0, math.inf, "(low, high) with 1 <= low <= high < inf")
        if self.ratio[1] == math.inf:
            raise ValueError(f"ratio must be (low, high) with 1 <= low <= high < inf, got {ratio}; p_limiter draws the infinite one")
        self.knee_db = _pair("knee_db", knee_db, 0.0, math.inf, "(low, high) with 0 <= low <= high < inf")
        self.makeup = _pair("makeup", makeup, 0.0, math.inf, "(low, high) with 0 <= low <= high < inf")
        for name, pair in (("knee_db", self.knee_db), ("makeup", self.makeup)):
            if pair[1] == math.inf:
                raise ValueError(f"{name} must be (low, high) with 0 <= low <= high < inf, got {pair}")
        self.attack_ms, self.release_ms = _positive_pair("attack_ms", attack_ms), _positive_pair("release_ms", release_ms)
        self.generator = generator

    def draw(self, B: int, fs: int, device=None) -> torch.Tensor:
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        u = torch.rand(B, 8, dtype=torch.float64, generator=gen, device=device)
        log_uniform = lambda r, v: torch.exp(math.log(r[0]) + (math.log(r[1]) - math.log(r[0])) * v)
        uniform = lambda r, v: r[0] + (r[1] - r[0]) * v
        ratio = torch.where(u[:, 2] < self.p_limiter, torch.full_like(u[:, 3], math.inf), log_uniform(self.ratio, u[:, 3]))
        drawn = dynamics_params(uniform(self.threshold_rel_db, u[:, 1]), ratio, uniform(self.knee_db, u[:, 4]),
                                log_uniform(self.attack_ms, u[:, 5]), log_uniform(self.release_ms, u[:, 6]),
                                uniform(self.makeup, u[:, 7]), fs)
        chosen = (u[:, 0] < self.p)[:, None]
        keep = torch.tensor([True, False, True, True, True, False]).to(device, non_blocking=True)   # an unchosen row: slope 0, m 0
        return torch.where(chosen | keep, drawn, torch.zeros_like(drawn))

    @staticmethod
    def table(drawn: torch.Tensor, wav: torch.Tensor) -> torch.Tensor:
        """The float64 [B, 6] table of Engine.dynamics for the float32 [B, L] batch `wav` and a `draw`."""
        top = wav.abs().amax(dim=1).to(torch.float64)
        on = torch.isfinite(top) & (top > 0)
        thr_rel, slope, knee, a_att, a_rel, m = drawn.unbind(dim=1)
        thr = 20.0 * torch.log10(torch.where(on, top, torch.ones_like(top))) + thr_rel
        slope = torch.where(on, slope, torch.zeros_like(slope))
        makeup = m * slope * torch.clamp(-thr_rel, min=0.0)              # peak_db - thr_db = -threshold_rel_db
        return torch.stack([thr, slope, knee, a_att, a_rel, makeup], dim=1).contiguous()


# ---- transmission: codec, bursty packet loss and concealment per row, as tables of Engine.transmit --------------------------
class TransmitDraw(NamedTuple):
    """What a TransmissionSampler drew for a batch, device tensors: the tables of Engine.transmit and what they came from."""
    lost: torch.Tensor        # uint8 [B, n_frames]: 1 where the frame is lost
    codec: torch.Tensor       # int32 [B]: 0 none, 1 16-bit PCM, 2 mu-law, 3 A-law
    plc: torch.Tensor         # int32 [B]: 1 conceal, 0 leave gaps
    rate: torch.Tensor        # float64 [B]: the mean loss of the row's chain (0 for a row that was not chosen)
    burst: torch.Tensor       # float64 [B]: its mean burst length in frames, raised to 1 / (1 - rate) where it was smaller


class TransmitInfo(NamedTuple):
    """`DynamicMixer.last_transmission`: the draw, and what Engine.transmit reported for `noisy` (status int32 [B], lag int32
    [B, n_frames]) and, with transmission_on="both", the lags of `target` (None otherwise)."""
    draw: TransmitDraw
    status: torch.Tensor
    lag: torch.Tensor
    target_lag: Optional[torch.Tensor] = None


class TransmissionSampler:
    """Random telephone / VoIP links for Engine.transmit: `draw(B, n_frames, device)` -> `TransmitDraw(lost, codec, plc, rate,
    burst)`.

    Per row, with probability `p`, a link: a mean loss `rate` uniform in `loss` (fractions in [0, 1)), a mean burst length
    uniform in `burst` (frames, >= 1), a codec - 16-bit PCM, mu-law or A-law with probabilities `p_pcm16`, `p_ulaw`,
    `p_alaw` (their sum at most 1), none otherwise - and a receiver that conceals with probability `p_conceal` (else
    it plays gaps).  A row that is not chosen has no loss, codec 0 and rate 0.  `frame_ms` is the packet length the
    mixer turns into Engine.transmit's `frame`.

    The loss pattern is a Gilbert-Elliott chain that starts in the good state, with mean loss `rate` and mean burst
    length `burst` frames: q = 1 / burst is the chance of leaving the bad state and p_gb = rate q / (1 - rate) that of
    entering it.  A burst shorter than 1 / (1 - rate) is raised to it: that limit is independent loss (p_gb = 1 - q =
    rate).  ONE uniform u_k per frame drives both states - u < p_gb: lost, whatever the state was; u >= 1 - q: received,
    whatever it was; in between the state stays - so frame k takes the verdict of the latest frame at or before it whose u
    falls outside the middle band (received with none): a cummax of an index, no loop (`pattern`).  Everything is drawn
    from `generator` (None: the device's default one) on the device with tensor arithmetic, one rand call of [B, 5 +
    n_frames] float64: no host synchronisation."""

    def __init__(self, p: float = 0.5, loss=(0.01, 0.2), burst=(1.0, 4.0), frame_ms: float = 20.0, p_conceal: float = 0.8,
                 p_pcm16: float = 0.2, p_ulaw: float = 0.2, p_alaw: float = 0.2, generator: Optional[torch.Generator] = None):
        self.p, self.p_conceal = _probability("p", p), _probability("p_conceal", p_conceal)
        self.p_pcm16, self.p_ulaw, self.p_alaw = (
            _probability(name, v) for name, v in (("p_pcm16", p_pcm16), ("p_ulaw", p_ulaw), ("p_alaw", p_alaw)))
        if self.p_pcm16 + self.p_ulaw + self.p_alaw > 1.0 + 1e-12:
            raise ValueError(f"p_pcm16 + p_ulaw + p_alaw must not exceed 1, got {self.p_pcm16 + self.p_ulaw + self.p_alaw}")
        self.loss = _pair("loss", loss, 0.0, 1.0, "(low, high) fractions with 0 <= low <= high < 1")
        if self.loss[1] >= 1.0:
            raise ValueError(f"loss must be (low, high) fractions with 0 <= low <= high < 1, got {loss}")
        self.burst = _pair("burst", burst, 1.0, math.inf, "(low, high) frames with 1 <= low <= high < inf")
        if self.burst[1] == math.inf:
            raise ValueError(f"burst must be (low, high) frames with 1 <= low <= high < inf, got {burst}")
        if isinstance(frame_ms, bool) or not isinstance(frame_ms, (int, float)) or not 0.0 < frame_ms < math.inf:
            raise ValueError(f"frame_ms must be a packet length > 0 in milliseconds, got {frame_ms}")
        self.frame_ms, self.generator = float(frame_ms), generator

    def frame(self, fs: int) -> int:
        """The packet length in samples at `fs`."""
        return int(round(self.frame_ms * fs / 1000.0))

    @staticmethod
    def pattern(u: torch.Tensor, p_gb: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
        """The chain's closed form: uint8 [B, n] from uniforms u [B, n] and the rows' p_gb and q [B]."""
        B, n = u.shape
        lose, keep = u < p_gb[:, None], u >= (1.0 - q)[:, None]
        k = torch.arange(n, device=u.device)[None, :].expand(B, n)
        last = torch.cummax(torch.where(lose | keep, k, torch.full_like(k, -1)), dim=1).values if n else k
        verdict = torch.gather(lose, 1, last.clamp(min=0))
        return ((last >= 0) & verdict).to(torch.uint8)

    def draw(self, B: int, n_frames: int, device=None) -> TransmitDraw:
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        u = torch.rand(B, 5 + int(n_frames), dtype=torch.float64, generator=gen, device=device)
        uniform = lambda r, v: r[0] + (r[1] - r[0]) * v
        chosen = u[:, 0] < self.p
        rate = torch.where(chosen, uniform(self.loss, u[:, 1]), torch.zeros_like(u[:, 1]))
        burst = torch.maximum(uniform(self.burst, u[:, 2]), 1.0 / (1.0 - rate))
        q = 1.0 / burst
        p_gb = rate * q / (1.0 - rate)
        plc = (u[:, 3] < self.p_conceal).to(torch.int32)
        a, b, c = self.p_pcm16, self.p_pcm16 + self.p_ulaw, self.p_pcm16 + self.p_ulaw + self.p_alaw
        kind = (u[:, 4] < c).to(torch.int32) * (1 + (u[:, 4] >= a).to(torch.int32) + (u[:, 4] >= b).to(torch.int32))
        codec = kind * chosen.to(torch.int32)
        return TransmitDraw(self.pattern(u[:, 5:], p_gb, q).contiguous(), codec, plc, rate, burst)


# ---- suppression: the table of Engine.suppress from audio units, and a sampler of it ---------------------------------------
def suppress_n_fft(fs: int) -> int:
    """The transform size the mixer and the baseline use at `fs`: 512 below 32 kHz (32 ms at 16 kHz), 1024 from there."""
    return 512 if fs < 32000 else 1024


def suppress_params(rule, floor_db=-20.0, bias=1.5, a_dd=0.98, a_n=0.8, window_s=1.0, xi_min_db=-25.0, fs=16000,
                    n_fft: Optional[int] = None) -> torch.Tensor:
    """The float64 [..., 7] table of Engine.suppress, (rule, a_dd, a_n, D, bias, g_min, xi_min) per row, from audio units:
    `rule` is "off", "wiener", "specsub" or "logmmse" (SUPPRESS_RULES; or a tensor of the codes 0 .. 3), g_min =
    10^(floor_db / 20) is the largest attenuation, D = round(window_s fs / (n_fft / 2)) frames the minimum search looks back
    over, kept inside 1 .. 128, xi_min = 10^(xi_min_db / 10); bias, a_dd and a_n go in as they are.  n_fft None: the size
    suppress_n_fft(fs) gives.  Plain float64 tensor arithmetic on the device of its arguments; what the result allows is
    judged per row by the kernels."""
    if isinstance(rule, str):
        if rule not in SUPPRESS_RULES:
            raise ValueError(f"rule must be one of {tuple(SUPPRESS_RULES)}, got {rule!r}")
        rule = float(SUPPRESS_RULES[rule])
    if not _whole_in(fs, 1, 2 ** 31 - 1):
        raise ValueError(f"fs must be a sample rate (a whole number >= 1), got {fs}")
    n_fft = suppress_n_fft(int(fs)) if n_fft is None else n_fft
    if isinstance(n_fft, bool) or n_fft not in SUPPRESS_N_FFT:
        raise ValueError(f"n_fft must be one of {SUPPRESS_N_FFT}, got {n_fft}")
    like = next((v for v in (rule, floor_db, bias, a_dd, a_n, window_s, xi_min_db) if isinstance(v, torch.Tensor)), None)
    rule, floor, bias, a_dd, a_n, window, xi = (_f64(v, like) for v in (rule, floor_db, bias, a_dd, a_n, window_s, xi_min_db))
    D = torch.clamp(torch.round(window * (float(fs) / (n_fft // 2))), 1.0, float(SUPPRESS_MAX_WINDOW))
    cols = torch.broadcast_tensors(rule, a_dd, a_n, D, bias, torch.pow(10.0, floor / 20.0), torch.pow(10.0, xi / 10.0))
    return torch.stack(cols, dim=-1).contiguous()


class SuppressDraw(NamedTuple):
    """What a SuppressorSampler drew for a batch: the float64 [B, 7] table of Engine.suppress and its n_fft."""
    table: torch.Tensor
    n_fft: int


class SuppressorSampler:
    """Random noise suppressors for Engine.suppress: `draw(B, fs, device)` -> `SuppressDraw(table, n_fft)`.

    Per row, with probability `p`, a suppressor: the rule - Wiener, power spectral subtraction or log-MMSE with
    probabilities `p_wiener`, `p_specsub` and the rest (their sum at most 1) - a gain floor uniform in `floor_db` (dB, at
    most 0), a noise over-estimation `bias` uniform in (0, 16], the decision-directed smoothing `a_dd` and the periodogram
    smoothing `a_n` uniform in their ranges inside [0, 1), and a minimum-search window uniform in `window_s` seconds;
    `xi_min_db` is one value for all.  A row that is not chosen gets rule 0, which Engine.suppress copies bit for bit; its
    other entries stay valid.  n_fft is suppress_n_fft(fs).  Everything is drawn from `generator` (None: the device's default
    one) on the device with tensor arithmetic, one rand call of [B, 7] float64: no host synchronisation."""

    def __init__(self, p: float = 0.5, p_wiener: float = 1.0 / 3.0, p_specsub: float = 1.0 / 3.0, floor_db=(-25.0, -6.0),
                 bias=(1.0, 3.0), a_dd=(0.9, 0.99), window_s=(0.4, 1.5), a_n=(0.7, 0.9), xi_min_db: float = -25.0,
                 generator: Optional[torch.Generator] = None):
        self.p, self.p_wiener, self.p_specsub = (
            _probability(name, v) for name, v in (("p", p), ("p_wiener", p_wiener), ("p_specsub", p_specsub)))
        if self.p_wiener + self.p_specsub > 1.0 + 1e-12:
            raise ValueError(f"p_wiener + p_specsub must not exceed 1, got {self.p_wiener + self.p_specsub}")
        self.floor_db = _pair("floor_db", floor_db, -math.inf, 0.0, "(low, high) dB with -inf < low <= high <= 0")
        if self.floor_db[0] == -math.inf:
            raise ValueError(f"floor_db must be (low, high) dB with -inf < low <= high <= 0, got {floor_db}")
        self.bias = _pair("bias", bias, 0.0, 16.0, "(low, high) with 0 < low <= high <= 16")
        if self.bias[0] <= 0.0:
            raise ValueError(f"bias must be (low, high) with 0 < low <= high <= 16, got {bias}")
        self.a_dd, self.a_n = (_pair(name, v, 0.0, 1.0, "(low, high) with 0 <= low <= high < 1") for name, v in (("a_dd", a_dd), ("a_n", a_n)))
        for name, pair, given in (("a_dd", self.a_dd, a_dd), ("a_n", self.a_n, a_n)):
            if pair[1] >= 1.0:
                raise ValueError(f"{name} must be (low, high) with 0 <= low <= high < 1, got {given}")
        self.window_s = _positive_pair("window_s", window_s)
        if isinstance(xi_min_db, bool) or not isinstance(xi_min_db, (int, float)) or not -math.inf < xi_min_db <= 0.0:
            raise ValueError(f"xi_min_db must be a finite level <= 0 in dB, got {xi_min_db}")
        self.xi_min_db, self.generator = float(xi_min_db), generator

    def draw(self, B: int, fs: int, device=None) -> SuppressDraw:
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        u = torch.rand(B, 7, dtype=torch.float64, generator=gen, device=device)
        uniform = lambda r, v: r[0] + (r[1] - r[0]) * v
        a, b = self.p_wiener, self.p_wiener + self.p_specsub
        rule = 1.0 + (u[:, 1] >= a).to(torch.float64) + (u[:, 1] >= b).to(torch.float64)
        rule = torch.where(u[:, 0] < self.p, rule, torch.zeros_like(rule))
        n_fft = suppress_n_fft(int(fs))
        table = suppress_params(rule, uniform(self.floor_db, u[:, 2]), uniform(self.bias, u[:, 3]), uniform(self.a_dd, u[:, 4]),
                                uniform(self.a_n, u[:, 6]), uniform(self.window_s, u[:, 5]), self.xi_min_db, fs, n_fft)
        return SuppressDraw(table, n_fft)


# ---- synthetic noise: the colouring filter of Engine.noise from a magnitude, and a sampler of its tables ----------------
NOISE_GRID = 4096             # points of the frequency grid the magnitudes are given on: [N, NOISE_GRID / 2 + 1]
NOISE_MAX_TAPS = 1023         # = cmgan_noise_max_filter()
NOISE_MAX_TONES = 8           # = cmgan_noise_max_tones()
NOISE_MAX_POINTS = 4096       # = cmgan_noise_max_points()


def power_law_magnitude(slope_db_per_octave, fs, f_lo: float = 62.5, band=None) -> torch.Tensor:
    """The magnitude (max(f, f_lo) / 1 kHz)^(slope / 6.0206) on the grid of `noise_fir`, f = i fs / 4096 for i = 0 .. 2048:
    float64 [..., 2049] for a slope of shape [...], in dB per octave of AMPLITUDE - -3 is pink, -6 brown, 0 white.  Below
    f_lo the law is held, so that a falling one stays finite at DC.  band=(lo, hi) in Hz (floats or tensors of the slope's
    shape) multiplies by raised-cosine edges on the octave scale, half an octave wide and centred on lo and hi.  Plain
    float64 tensor arithmetic on the device of its arguments, like the biquad designs."""
    slope = _f64(slope_db_per_octave)
    fs, f_lo = float(fs), float(f_lo)
    if not (0.0 < fs < math.inf and 0.0 < f_lo < math.inf):
        raise ValueError(f"fs and f_lo must be positive and finite, got fs = {fs}, f_lo = {f_lo}")
    f = torch.arange(NOISE_GRID // 2 + 1, dtype=torch.float64).to(slope.device, non_blocking=True) * (fs / NOISE_GRID)
    mag = torch.exp2(torch.log2(torch.clamp(f, min=f_lo) / 1000.0) * (slope[..., None] / (20.0 * math.log10(2.0))))
    if band is not None:
        lo, hi = (_f64(v, slope)[..., None] for v in band)
        u = torch.log2(torch.clamp(f, min=1e-300))               # (-996 at DC: below every lower edge)
        rise = torch.clamp((u - torch.log2(lo) + 0.25) / 0.5, 0.0, 1.0)
        fall = torch.clamp((u - torch.log2(hi) + 0.25) / 0.5, 0.0, 1.0)
        mag = mag * (0.5 - 0.5 * torch.cos(math.pi * rise)) * (0.5 + 0.5 * torch.cos(math.pi * fall))
    return mag


def noise_fir(magnitude: torch.Tensor, n_taps: int) -> torch.Tensor:
    """The colouring filter of Engine.noise by frequency sampling: float64 [N, n_taps] from `magnitude`, float64 [N, 2049]
    on the 4096-point grid (bin i at i fs / 4096).  The zero-phase inverse real FFT is centred at (n_taps - 1) // 2, cut to
    n_taps taps, multiplied by the Hann window 0.5 - 0.5 cos(2 pi (i + 1) / (n_taps + 1)) and normalised to sum h^2 = 1, so
    that the filtered unit-variance noise has unit variance whatever its colour.  A row whose taps are all zero stays
    zero.  Plain float64 tensor arithmetic on the device of `magnitude`."""
    if not isinstance(magnitude, torch.Tensor) or magnitude.dtype != torch.float64 or magnitude.dim() != 2 \
            or magnitude.size(1) != NOISE_GRID // 2 + 1:
        raise ValueError(f"magnitude must be a float64 [N, {NOISE_GRID // 2 + 1}] tensor on the {NOISE_GRID}-point grid")
    if not _whole_in(n_taps, 1, NOISE_MAX_TAPS):
        raise ValueError(f"n_taps must be a whole number in [1, {NOISE_MAX_TAPS}], got {n_taps}")
    NF = int(n_taps)
    j = torch.arange(NF, dtype=torch.int64).to(magnitude.device, non_blocking=True)
    h = torch.fft.irfft(magnitude.to(torch.complex128), n=NOISE_GRID, dim=1)[:, (j - (NF - 1) // 2) % NOISE_GRID]
    h = h * (0.5 - 0.5 * torch.cos(2.0 * math.pi * (j + 1).to(torch.float64) / (NF + 1)))
    norm = torch.sqrt((h * h).sum(dim=1, keepdim=True))
    return (h / torch.where(norm > 0, norm, torch.ones_like(norm))).contiguous()


class NoiseDraw(NamedTuple):
    """NoiseSampler.draw: the tables of Engine.noise for N rows, all on the device.  seed int64 [N]; fir float64 [N,
    n_taps]; env float64 [N, P], the gain at points `NoiseSampler.hop(fs)` samples apart; tones float64 [N, M, 3] and n_tones
    int32 [N] (None with p_hum = 0); impulse float64 [N, 2] (None with p_clicks = 0)."""
    seed: torch.Tensor
    fir: torch.Tensor
    env: torch.Tensor
    tones: Optional[torch.Tensor]
    n_tones: Optional[torch.Tensor]
    impulse: Optional[torch.Tensor]


class NoiseSampler:
    """Random noises for Engine.noise: `draw(N, n, fs, device)` -> a NoiseDraw for N rows of n samples.

    Per row: a spectrum - a power law with the slope uniform in `slope_db` (dB per octave: -3 pink, -6 brown, 0 white),
    with `band_hz` = (lo, hi) also a band whose two edges are log-uniform in its lower and upper half on the octave
    scale - designed into `n_taps` taps by `noise_fir`; an envelope 10^(d(t) / 20) at points `env_hop_ms` apart, d the sum
    of three sinusoids with rates log-uniform in `mod_rate_hz` and uniform phases, scaled so that the largest |d| of the
    row's points is a depth uniform in `mod_depth_db`; with probability `p_hum` a hum - a fundamental chosen from `hum_hz`
    with equal probability, a number of harmonics uniform in `hum_harmonics` (whole numbers, at most 8; those above fs / 2
    are dropped), each 6 dB below the one before, the fundamental's RMS uniform in `hum_db` relative to the unit-variance
    noise, phases uniform; with probability `p_clicks` clicks - `click_rate_hz` (log-uniform) of them per second on
    average, their amplitude uniform in +-10^(click_db / 20), `click_db` uniform and relative to the noise's RMS; they pass
    the row's filter like the noise.  Everything is drawn from `generator` (None: the device's default one) on the
    device with tensor arithmetic: no host synchronisation.  No row of a draw is invalid."""

    def __init__(self, slope_db=(-9.0, 3.0), band_hz=None, mod_depth_db=(0.0, 12.0), mod_rate_hz=(0.5, 8.0), p_hum: float = 0.2,
                 hum_hz=(50.0, 60.0), hum_db=(-30.0, -10.0), hum_harmonics=(1, 5), p_clicks: float = 0.1,
                 click_rate_hz=(1.0, 20.0), click_db=(10.0, 30.0), n_taps: int = 255, env_hop_ms: float = 20.0,
                 generator: Optional[torch.Generator] = None):
        finite = "(low, high) with finite low <= high"
        self.slope_db = _pair("slope_db", slope_db, -math.inf, math.inf, finite, closed=False)
        self.band_hz = None if band_hz is None else _positive_pair("band_hz", band_hz, "None or (low, high)")
        self.mod_depth_db = _pair("mod_depth_db", mod_depth_db, 0.0, math.inf, "(low, high) with 0 <= low <= high < inf")
        if self.mod_depth_db[1] == math.inf:
            raise ValueError(f"mod_depth_db must be (low, high) with 0 <= low <= high < inf, got {mod_depth_db}")
        self.mod_rate_hz = _positive_pair("mod_rate_hz", mod_rate_hz)
        self.p_hum, self.p_clicks = _probability("p_hum", p_hum), _probability("p_clicks", p_clicks)
        try:
            self.hum_hz = tuple(float(f) for f in hum_hz)
        except (TypeError, ValueError):
            self.hum_hz = ()
        if not self.hum_hz or not all(0.0 < f < math.inf for f in self.hum_hz):
            raise ValueError(f"hum_hz must be one or more positive frequencies to choose from, got {hum_hz}")
        self.hum_db = _pair("hum_db", hum_db, -math.inf, math.inf, finite, closed=False)
        counts = f"(low, high) whole numbers with 1 <= low <= high <= {NOISE_MAX_TONES}"
        self.hum_harmonics = _pair("hum_harmonics", hum_harmonics, 1, NOISE_MAX_TONES, counts, whole=True)
        self.click_rate_hz = _positive_pair("click_rate_hz", click_rate_hz)
        self.click_db = _pair("click_db", click_db, -math.inf, math.inf, finite, closed=False)
        if not _whole_in(n_taps, 1, NOISE_MAX_TAPS):
            raise ValueError(f"n_taps must be a whole number in [1, {NOISE_MAX_TAPS}], got {n_taps}")
        if isinstance(env_hop_ms, bool) or not isinstance(env_hop_ms, (int, float)) or not 0.0 < env_hop_ms < math.inf:
            raise ValueError(f"env_hop_ms must be a positive, finite number of milliseconds, got {env_hop_ms}")
        self.n_taps, self.env_hop_ms, self.generator = int(n_taps), float(env_hop_ms), generator

    def hop(self, fs: int) -> int:
        """H, the samples between two points of the envelope: env_hop_ms at fs, rounded, at least 1 (Engine.noise's env_hop)."""
        return max(1, int(round(self.env_hop_ms * float(fs) / 1000.0)))

    def points(self, n: int, fs: int) -> int:
        """P, the envelope points that n samples from index 0 reach: 2 + (n - 1) div H; more than 4096 is refused."""
        P = 2 + max(int(n) - 1, 0) // self.hop(fs)
        if P > NOISE_MAX_POINTS:
            raise ValueError(f"{n} samples with an envelope point every {self.hop(fs)} need {P} points; up to {NOISE_MAX_POINTS} "
                             f"are supported: raise env_hop_ms")
        return P

    def draw(self, N: int, n: int, fs: int, device=None) -> NoiseDraw:
        gen = self.generator
        device = torch.device(device) if device is not None else (gen.device if gen is not None else torch.device("cpu"))
        fs = float(fs)
        H, P, M = self.hop(fs), self.points(n, fs), self.hum_harmonics[1]
        if self.band_hz is not None and not self.band_hz[1] <= 0.5 * fs:
            raise ValueError(f"band_hz = {self.band_hz} must lie at or below fs / 2 = {0.5 * fs} Hz")
        seed = torch.randint(0, 2 ** 63 - 1, (N,), dtype=torch.int64, generator=gen, device=device)
        u = torch.rand(N, 17 + M, dtype=torch.float64, generator=gen, device=device)
        uniform = lambda r, v: r[0] + (r[1] - r[0]) * v
        log_uniform = lambda r, v: torch.exp(math.log(r[0]) + (math.log(r[1]) - math.log(r[0])) * v)
        # ---- the spectrum
        band = None
        if self.band_hz is not None:
            lo, hi = self.band_hz
            mid = math.sqrt(lo * hi)
            band = (log_uniform((lo, mid), u[:, 1]), log_uniform((mid, hi), u[:, 2]))
        fir = noise_fir(power_law_magnitude(uniform(self.slope_db, u[:, 0]), fs, band=band), self.n_taps)
        # ---- the envelope
        t = torch.arange(P, dtype=torch.float64).to(device, non_blocking=True) * (H / fs)
        rate, phase = log_uniform(self.mod_rate_hz, u[:, 3:6]), u[:, 6:9]
        d = torch.sin(2.0 * math.pi * (rate[:, :, None] * t[None, None, :] + phase[:, :, None])).sum(dim=1)
        top = d.abs().amax(dim=1, keepdim=True)
        d = d / torch.where(top > 0, top, torch.ones_like(top)) * uniform(self.mod_depth_db, u[:, 9])[:, None]
        env = torch.pow(10.0, d / 20.0).contiguous()
        # ---- the hum
        tones = n_tones = None
        if self.p_hum > 0.0:
            choice = torch.tensor(self.hum_hz, dtype=torch.float64).to(device, non_blocking=True)
            f0 = choice[torch.clamp((u[:, 11] * len(self.hum_hz)).to(torch.int64), max=len(self.hum_hz) - 1)]
            lo, hi = self.hum_harmonics
            count = lo + torch.clamp((u[:, 12] * (hi - lo + 1)).to(torch.int64), max=hi - lo)
            m = torch.arange(M, dtype=torch.float64).to(device, non_blocking=True)
            nu = f0[:, None] * (m[None, :] + 1.0) / fs
            amp = (math.sqrt(2.0) * torch.pow(10.0, uniform(self.hum_db, u[:, 13]) / 20.0))[:, None] * torch.exp2(-m)[None, :]
            audible = (nu <= 0.5).sum(dim=1)                      # (nu rises with m: the audible harmonics come first)
            n_tones = torch.where(u[:, 10] < self.p_hum, torch.minimum(count, audible), torch.zeros_like(count)).to(torch.int32)
            tones = torch.stack([torch.clamp(nu, max=0.5), amp, u[:, 17:17 + M]], dim=2).contiguous()
        # ---- the clicks
        impulse = None
        if self.p_clicks > 0.0:
            thr = torch.clamp(torch.floor(log_uniform(self.click_rate_hz, u[:, 14]) / fs * 2.0 ** 32), 0.0, 2.0 ** 32 - 1.0)
            thr = torch.where(u[:, 15] < self.p_clicks, thr, torch.zeros_like(thr))
            impulse = torch.stack([thr, torch.pow(10.0, uniform(self.click_db, u[:, 16]) / 20.0)], dim=1).contiguous()
        return NoiseDraw(seed, fir, env, tones, n_tones, impulse)


class RirBank:
    """Room impulse responses as one float32 [R, Kmax] device allocation, rows zero-padded, plus `length` (int32 [R]).
    Recorded responses come from `from_dir` / `from_arrays`; `simulate` makes the bank on the device from random shoe-box
    rooms (Engine.rir, the image-source method) and keeps their table as `rooms` (float64 [R, 15], else None); with a
    banded sampler (RoomSampler(bands=n): Engine.rir_bands) also their band table as `bands` (float64 [R, n, 7]).
    With a directional sampler (RoomSampler(source_pattern=, mic_pattern=)) `orient` and `pattern` keep its draw_dirs.
    `measure` leaves what the responses measure as in `stats` (a RirStats of [R, NB + 1] tensors, else None), and `where`
    selects rows by it."""

    def __init__(self, data: torch.Tensor, length: torch.Tensor, rooms: Optional[torch.Tensor] = None,
                 bands: Optional[torch.Tensor] = None, stats: Optional[RirStats] = None):
        self.data, self.length, self.rooms, self.bands, self.stats = data, length, rooms, bands, stats
        self.tail: Optional[RirTail] = None      # simulate with RoomSampler(tail_ms=...): the fitted levels and the status
        self.orient = self.pattern = None        # simulate with a directional RoomSampler: the tables of its draw_dirs

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
    def simulate(cls, engine, sampler: RoomSampler, R: int, seconds: float = 0.5, sample_rate: int = 16000,
                 measure: bool = False) -> "RirBank":
        """R rooms drawn by `sampler`, each simulated for up to `seconds` (a row's own length is its rt60, if shorter).
        With RoomSampler(tail_ms=...) the image-source call stops at each row's junction and Engine.rir_tail adds the
        rest (`tail` keeps its RirTail).  measure=True then measures the bank (`measure`), in the sampler's bands if it
        has any."""
        K = int(round(seconds * sample_rate))
        rooms, n_taps = sampler.draw(R, K, sample_rate, device=engine.device)
        N = sampler.n_images(K, sample_rate)
        filters = None if sampler.bands is None else sampler.filters(sample_rate, engine.device)
        bands = None if filters is None else sampler.draw_bands(rooms)
        t = None if sampler.tail_ms is None else sampler.draw_tail(rooms, sample_rate)
        orient, pattern = sampler.draw_dirs(rooms) if sampler.directional else (None, None)      # (after every other draw)
        if filters is None:
            bank = cls(*engine.rir(rooms, n_taps, K, N, fs=sample_rate, orient=orient, pattern=pattern), rooms)
        else:
            bank = cls(*engine.rir_bands(rooms, bands, n_taps, K, filters, N, fs=sample_rate, orient=orient, pattern=pattern),
                       rooms, bands)
        bank.orient, bank.pattern = orient, pattern
        if t is not None:                                         # the responses end at their junctions: the diffuse tail
            bank.tail = engine.rir_tail(bank.data, bank.length, t.n_full, t.decay, t.seed, filters, fs=sample_rate,
                                        window_ms=sampler.tail_window_ms)[2]
        if measure:
            bank.measure(engine, sample_rate, filters)
        return bank

    def measure(self, engine, fs: int = 16000, filters: Optional[torch.Tensor] = None) -> RirStats:
        """What every response measures as (Engine.rir_stats: EDT, T20, T30, DRR, C50, ... broad-band and, with `filters`
        = float64 [NB, NF] on the device, per band), kept as `self.stats` and returned.  No host synchronisation."""
        self.stats = engine.rir_stats(self.data, self.length, filters, fs=fs)
        return self.stats

    def where(self, t30=None, drr_db=None, c50_db=None, band: int = 0) -> "RirBank":
        """The sub-bank of the rows whose measured T30, DRR and C50 of column `band` (0: broad-band, 1 + b: band b) lie in
        the given closed (low, high) ranges (None: not asked): `data`, `length`, `rooms`, `bands` and `stats`
        index-selected on the device, in their order.  A NaN never lies in a range, so a row whose T30 could not be
        fitted is dropped when `t30` is asked.  The bank must have been measured.  This is a bank-building step: the row
        count of the result is read back from the device, ONE host synchronisation; an empty selection is an error."""
        if self.stats is None:
            raise ValueError("where() needs a measured bank: call measure() first, or simulate(..., measure=True)")
        columns = self.stats.t30.size(1)
        if isinstance(band, bool) or int(band) != band or not 0 <= band < columns:
            raise ValueError(f"band must be a column in [0, {columns - 1}] of the measured stats, got {band}")
        keep = torch.ones(len(self), dtype=torch.bool, device=self.device)
        for name, rng, field in (("t30", t30, self.stats.t30), ("drr_db", drr_db, self.stats.drr_db),
                                 ("c50_db", c50_db, self.stats.c50_db)):
            if rng is not None:
                lo, hi = _pair(name, rng, -math.inf, math.inf, "(low, high) with low <= high", "None or (low, high)")
                keep &= (field[:, int(band)] >= lo) & (field[:, int(band)] <= hi)
        index = torch.nonzero(keep).squeeze(1)                    # (the synchronisation)
        if index.numel() == 0:
            raise ValueError(f"where(t30={t30}, drr_db={drr_db}, c50_db={c50_db}, band={band}) selects no row of {len(self)}")
        pick = lambda t: None if t is None else t.index_select(0, index).contiguous()
        return RirBank(pick(self.data), pick(self.length), pick(self.rooms), pick(self.bands), RirStats(*map(pick, self.stats)))

    def with_identity(self) -> "RirBank":
        """The bank with a one-tap identity response appended as its last row (rows that get no reverberation).  A
        measured bank stays one: the row measures as cmgan_rir_stats defines a lone unit sample - energy 1, direct 0, no
        reverberant part (DRR, C50, C80 +inf; D50 1; Ts 0) and no decay to fit (NaN, the three bits) - in every column."""
        row = torch.zeros(1, self.data.size(1), dtype=torch.float32, device=self.device)
        row[0, 0] = 1.0
        one = torch.ones(1, dtype=torch.int32, device=self.device)
        stats = self.stats
        if stats is not None:
            inf, nan = math.inf, math.nan
            lone = RirStats(1.0, 0.0, inf, inf, inf, 1.0, 0.0, nan, nan, nan, 4 | 8 | 16)
            stats = RirStats(*(torch.cat([t, torch.full_like(t[:1], v)]) for t, v in zip(stats, lone)))
        return RirBank(torch.cat([self.data, row]).contiguous(), torch.cat([self.length, one]), stats=stats)


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
    channel: Optional[tuple] = None           # DynamicMixer(channel=...): (sos, n_sections, n_shared, clip_rel) of the batch
    speed: Optional[torch.Tensor] = None      # DynamicMixer(speed=...): the float64 [B] rate of Engine.warp per row


class StretchDraw(NamedTuple):
    """What a DynamicMixer(tempo=..., pitch=...) drew for a batch, float64 [B] device tensors: the tempo t, the pitch
    factor p = 2^(semitones / 12), and the rates of the two calls they give with the speed v of Draw.speed (1 without
    `speed`): Engine.stretch at t / p, then Engine.warp at v p (None when no warp runs: `tempo` alone, without `speed`)."""
    tempo: torch.Tensor
    pitch_factor: torch.Tensor
    stretch_rate: torch.Tensor
    warp_rate: Optional[torch.Tensor]


_SOURCE_FIELDS = (
    "n_src",                                      # int32 [B]: how many of the S columns a row uses
    "src_start", "src_len", "src_off", "src_snr_db",
    "src_rir_index", "src_rir_len",               # None without a rir_bank or rooms: the sources are dry
    "src_rooms",                                  # with rooms=...: the float64 [B, S, 15] tables of RoomSampler.draw_sources
)
SceneDraw = collections.namedtuple("SceneDraw", Draw._fields + _SOURCE_FIELDS,
                                   defaults=(None,) * (len(Draw._field_defaults) + len(_SOURCE_FIELDS)))
SceneDraw.__doc__ = """What a DynamicMixer(sources=...) drew for a batch: the fields of Draw, then the per-source arguments of
Engine.scene, [B] and [B, S] device tensors with S = the upper end of `sources`."""


_PATH_FIELDS = (
    "path",                                       # float64 [B, P, 15]: RoomSampler.draw_path of the batch's rooms (None: the talkers stand still)
    "n_path",                                     # int32 [B]: P for a row that moves, 1 for one drawn static
    "src_path", "src_n_path",                     # float64 [B, S, P, 15] and int32 [B, S] (None without sources; src_path None: they stand still)
)
PathDraw = collections.namedtuple("PathDraw", SceneDraw._fields + _PATH_FIELDS,
                                  defaults=(None,) * (len(SceneDraw._field_defaults) + len(_PATH_FIELDS)))
PathDraw.__doc__ = """What a DynamicMixer(motion=... / source_motion=...) drew for a batch: the fields of SceneDraw (the sources' None
without `sources`), then the paths.  rir_index / rir_len are the [B, P] and src_rir_index / src_rir_len the [B, S, P] tables
of Engine.scene_path.  Draw and SceneDraw keep their fields: a mixer without motion never makes a PathDraw."""


# DynamicMixer(dynamics=...): the float64 [B, 6] table of Engine.dynamics the batch went through, as `last_draw.dynamics`.
# It is an attribute beside the fields, not one of them: the draws keep their fields, their order and their length.
Draw.dynamics = SceneDraw.dynamics = PathDraw.dynamics = None
_DYNAMICS_DRAWS = {cls: type(cls.__name__, (cls,), {"__doc__": cls.__doc__}) for cls in (Draw, SceneDraw, PathDraw)}


def _with_dynamics(d, table: torch.Tensor):
    """The draw `d` with `d.dynamics = table`."""
    out = _DYNAMICS_DRAWS[type(d)](*d)
    out.dynamics = table
    return out


class _Paths(NamedTuple):
    """The sampler's part of a PathDraw, before the responses are simulated: the tables and every waypoint's n_taps."""
    P: int
    path: Optional[torch.Tensor]
    taps: Optional[torch.Tensor]                  # int32 [B, P]
    src_path: Optional[torch.Tensor]
    src_taps: Optional[torch.Tensor]              # int32 [B, S, P]


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
    scaled row again gives a slightly different level than the one drawn.

    `channel` (a ChannelSampler): the recording channel (Engine.channel / cmgan_channel).  With None nothing is drawn or
    run and the outputs, `last_draw` and every generator state are what they are without the argument.  With a sampler, a
    channel per row is drawn after every other draw, from the sampler's own generator, and kept as `last_draw.channel`;
    `noisy` goes through the row's sections in place and is then limited to clip = clip_rel x max |noisy| of the row as it
    was BEFORE the channel (`channel_clip`; no limit where clip_rel is +inf or the row is silent).  `channel_on="noisy"`
    (the default) leaves the target as it is: the model is asked to undo the channel too.  `channel_on="both"` also passes
    `target` through the row's first n_shared sections, without clipping: the model is then not asked to undo the
    microphone or to extend the bandwidth.  The mixer's peak guard (`peak`) acts BEFORE the channel, so a boosting
    equaliser can exceed it; that is what the clip is for.

    `dynamics` (a DynamicsSampler): a gain control in the recording device - compressor, limiter, AGC (Engine.dynamics /
    cmgan_dynamics) - between the mix and the channel, whose clipping stays the last thing that happens to the signal.
    With None nothing is drawn or run and the outputs, `last_draw` and every generator state are what they are without
    the argument.  With a sampler, a processor per row is drawn after every other draw, from the sampler's own generator;
    its threshold is relative to max |noisy| of the row as the mix left it, and the table the kernels got stays readable
    as `last_draw.dynamics` (float64 [B, 6]; an attribute beside the draw's fields) and the largest gain reduction per row
    as `mixer.last_dynamics` (float64 [B], dB).  `dynamics_on="noisy"` (the default) processes `noisy` alone: the model is
    asked to undo the gain control too.  `dynamics_on="both"` first applies the gain that `noisy` drives to `target`
    (key=noisy), then processes `noisy`: the target carries the same gain trajectory and the task stays denoising.  A
    make-up gain can lift a row above `peak`; such a row's `noisy` and `target` are then scaled by peak / max |noisy|,
    the rule of Engine.mix's peak guard (every other row by exactly 1).

    `speed=(lo, hi)` with 1/4 <= lo <= hi <= 4: speed perturbation (Engine.warp / cmgan_warp), the one stage that changes
    the talker: tempo and pitch move together.  With None (the default) nothing is drawn or run and the outputs,
    `last_draw` (apart from its trailing `speed=None`) and every generator state are what they are without the argument.
    With a range, a float64 rate per row - input samples per output sample, > 1 is faster and higher - is drawn from the
    mixer's generator after the `level_db` draw: uniform in [lo, hi], and exactly 1.0 with probability 1 - `p_speed`;
    it is kept as `last_draw.speed`.  The clean batch goes through Engine.warp FIRST, before the level measurement and
    before Engine.mix, with n_out = N = warp_len(L, hi): every rate <= hi makes at least N outputs of L samples, so all
    rows are full and target and noisy are [B, N].  The loader should therefore cut clips hi times longer than the batch
    it wants: `clean_only(dir, cut_len=math.ceil(32000 * hi))` for batches of 32000.  A row drawn as 1.0 passes the same
    filter (`speed_zeros`, `speed_rolloff`) as the others - it is band-limited at the rolloff, not copied.

    `tempo=(lo, hi)` (rates, > 1 is faster) and `pitch=(lo, hi)` in SEMITONES, |.| <= 12: tempo and pitch perturbation, each
    on its own (Engine.stretch / cmgan_stretch: a WSOLA time stretch that keeps the pitch, tuned to speech - `stretch_hop`,
    `stretch_search` - and not meant for music).  With both None (the default) nothing is drawn or run and the outputs,
    `last_draw` and every generator state are what they are without the arguments; `Draw` and `SceneDraw` are the same
    either way.  Otherwise, per row and from the mixer's generator AFTER every other draw (the sources' included): a tempo
    t uniform in its range, or exactly 1.0 with probability 1 - `p_tempo`, and a pitch factor p = 2^(semitones / 12) with
    the semitones uniform in their range, or exactly 1.0 with probability 1 - `p_pitch`; they are kept, with the two rates
    below, as `mixer.last_stretch` (a StretchDraw; None when the stage is off).  With v the row's speed draw (1 without
    `speed`), the clean batch goes FIRST through Engine.stretch at rate t / p with n_out = N1 = warp_len(L, t_hi / p_lo),
    then through ONE Engine.warp at rate v p with n_out = warp_len(N1, v_hi p_hi): the stretch changes the duration by p / t
    at the pitch it has, the warp moves tempo and pitch together by v p, so the duration changes by 1 / (t v) and the
    pitch by v p.  The speed stage's own warp is folded into that one (otherwise the speed path is as it was), and with
    `tempo` alone, without `speed`, no warp runs.  Where a probability is below 1, the value 1.0 counts as part of its
    range in these bounds, so all rows come out full; target and noisy are [B, stretch_len(L, tempo, pitch, speed, ...)].
    The loader should cut clips of about N (t_hi / p_lo) (v_hi p_hi) samples for batches of N: pick the smallest L with
    stretch_len(L, ...) >= N.  Ranges whose rates t / p or v p can leave [1/4, 4] are refused.

    `sources=(lo, hi)` with 0 <= lo <= hi, 1 <= hi <= 4: point noise sources and interfering talkers INSIDE the room
    (Engine.scene / cmgan_scene).  With None (the default) the mixer calls Engine.mix and the outputs, `last_draw` (apart
    from its trailing `speed=None`) and every generator state are what they are without the argument: `last_draw` is a
    Draw.  With a range `last_draw` is a SceneDraw, Draw's fields followed by the sources' (None by default); each
    row gets a source count uniform in [lo, hi] and, for each of the S = hi table columns, an item and an offset of
    `source_bank` (a NoiseBank; None: the noise bank - a bank of speech gives interfering talkers) and a
    speech-to-source ratio uniform in `source_snr_db`; with `snr_on="active"` that ratio relates to the active speech
    power like `snr_db`.  These come from the mixer's generator after every other draw.  With a `rir_bank` every source
    draws a response of the bank (the identity of p_reverb excluded); with `rooms`, `RoomSampler.draw_sources` then draws
    every source a position in its row's room (from the sampler's generator, kept as `last_draw.src_rooms`) and ONE more
    Engine.rir call simulates the B S responses into the rows behind the talkers' (and the identity) of the same
    persistent bank; with neither the sources are dry.  A source keeps its room's own response length whether or not the
    talker's row was drawn dry, and its delay: it is not aligned with the talker.  The mixer then returns a SceneInfo.
    `dry_noise=False` (only with sources) drops the noise that is added without a room, so every noise is located; the
    noise draws are made as before and not used.

    `room_stats=True`: the batch is labelled with the acoustics it was mixed with (Engine.rir_stats / cmgan_rir_stats: T30,
    DRR, C50, ... of ISO 3382-1).  With `rooms` the talkers' B simulated responses are measured once per call, on the
    device, in the sampler's bands if it has any; with a `rir_bank` that has been measured (`RirBank.measure`) its `stats`
    are gathered by the drawn index (a dry row shows the identity's).  Either way `mixer.last_room_stats` is a RirStats
    of [B, NB + 1] tensors for the rows of the batch, a dry row of `rooms` showing its one-tap response.  Nothing is
    drawn for it: with False (the default) `last_room_stats` is None and the outputs, draws and generator states are
    what they are without the argument, and with True they are the same too.  An unmeasured bank, or neither a bank nor
    rooms, is refused.

    `noise` (a NoiseSampler, with `noise_bank` = None): no recorded noise at all.  Every call first synthesizes B rows of the
    length the batch will have (Engine.noise / cmgan_noise; the sampler draws from its own generator) into one persistent
    [B, N] allocation, overwritten in place, and installs it as `noise_bank`: the item, offset and SNR draws and every
    kernel behind them then run against it as against any bank, and `sources` without a `source_bank` takes its point
    noises from the same rows.  The sampler's draw stays readable as `mixer.last_noise`.  `noise` and a `noise_bank`
    together are refused, and so is neither.  With `noise=None` nothing is drawn or launched, and the outputs, `last_draw`
    and every generator state are what they are without the argument.

    `rooms=RoomSampler(tail_ms=...)`: the hybrid room simulator.  The image-source calls stop at every response's junction
    (the talkers' and each located source's own) and Engine.rir_tail / cmgan_rir_tail adds a diffuse tail up to the
    response's whole length, so `rir_seconds` of a second or two stay affordable.  The tail draw (`mixer.last_tail`, a
    TailDraw) follows `draw` and `draw_bands`; `last_draw.rir_len` and `src_rir_len` then hold the EXTENDED lengths the batch
    was mixed with, and `room_stats=True` measures the extended responses.  Without `tail_ms` nothing of this is drawn or
    run.

    `rooms=RoomSampler(source_pattern=..., mic_pattern=...)`: directional talkers and microphones (Engine.rir / rir_bands with
    orient= and pattern=).  RoomSampler.draw_dirs is called where the responses are simulated, after every other draw of the
    sampler: once for the talkers - on a path every waypoint keeps the walk's angle to the microphone - and once for the
    sources, which face any way (`facing_deg=(0, 180)` whatever the sampler's range); `mixer.last_dirs` keeps the two
    (orient, pattern) pairs.  Without the options nothing of this is drawn and the batch is bit-identical to before.

    `motion=(lo, hi)` metres per second (needs `rooms`; a `rir_bank` of fixed responses cannot move): talkers that walk
    (Engine.scene_path / cmgan_scene_path).  A waypoint every `motion_hop_ms` (H samples, `motion_hop`), P = 1 + ceil((N -
    1) / H) of them for the batch length N that reaches the mix, at most 64 (`waypoints(N)`).  Every row gets a path,
    `RoomSampler.draw_path` from its drawn source position over (P - 1) H samples, made from the sampler's generator
    after all its other draws, and all B P responses are simulated into the persistent bank by the calls a static batch
    makes (with `bands` the waypoints share their room's band table; with `tail_ms` every waypoint has a junction of its
    own, and all waypoints of a path share ONE tail seed and decay: their tails are the same noise at fitted levels, so
    the cross-fade does not dip by 3 dB between uncorrelated tails).  A row then moves with probability `p_motion`
    (n_path = P) or stands at waypoint 0 (n_path = 1): one rand(B) from the mixer's generator after every other draw,
    the stretch draws included.  `source_motion=(lo, hi)` (needs `sources` and `rooms`) walks every located source the
    same way, a path per source drawn after the talkers'.  `last_draw` is then a PathDraw and the mixer returns a
    SceneInfo.  `room_stats=True` measures waypoint 0 of every talker.  Doppler is not modelled.  With both None (the
    default) nothing is drawn or run: outputs, `last_draw` and every generator state are what they are without them.

    `transmission` (a TransmissionSampler): the link between the recording device and the listener (Engine.transmit /
    cmgan_transmit), the LAST stage, behind the channel: a codec, packets of `frame_ms` that are lost in bursts, and a
    receiver that conceals them or not.  With None nothing is drawn or launched, and the outputs, `last_draw` and every
    generator state are what they are without the argument.  With a sampler, a link per row is drawn after every other
    draw of the call, from the sampler's own generator, for the ceil(N / frame) packets of the batch, and `noisy` goes
    through it in place (lags, window and fade at Engine.transmit's defaults for `sample_rate`).  `transmission_on=
    "noisy"` (the default) leaves the target as it is: the model is asked to undo the link too.  `transmission_on="both"`
    also sends `target` through the same call with the same tables - it loses the same packets and conceals them from its
    OWN history - so the task stays denoising.  `mixer.last_transmission` is a TransmitInfo: the draw, and the status and
    lags the kernels reported.

    `suppressor` (a SuppressorSampler): the recording device's own single-channel noise suppressor (Engine.suppress /
    cmgan_suppress), between the channel and the link: what it leaves behind - musical noise, speech attenuated where the
    SNR is low, a floor that pumps with the estimate - is what most real "noisy" recordings carry.  With None nothing is
    drawn or launched, and the outputs, `last_draw` and every generator state are what they are without the argument.
    With a sampler, a suppressor per row is drawn after the dynamics draw and before the link's, from the sampler's own
    generator, and `noisy` goes through it in place at n_fft = suppress_n_fft(sample_rate).  `suppressor_on="noisy"` (the
    default) leaves the target as it is; `suppressor_on="both"` first gives `target` the gains that `noisy` drives (key =
    noisy), so the task stays denoising.  `mixer.last_suppression` is the SuppressDraw (table, n_fft)."""

    def __init__(self, engine, noise_bank: NoiseBank, rir_bank: Optional[RirBank] = None, snr_db=(0.0, 20.0),
                 early_ms: Optional[float] = 50.0, p_reverb: float = 1.0, peak: float = 0.99,
                 generator: Optional[torch.Generator] = None, sample_rate: int = 16000,
                 rooms: Optional[RoomSampler] = None, rir_seconds: float = 0.5, snr_on: str = "rms", level_db=None,
                 channel: Optional[ChannelSampler] = None, channel_on: str = "noisy", speed=None, p_speed: float = 1.0,
                 speed_zeros: int = 24, speed_rolloff: float = 0.95, sources=None, source_bank: Optional[NoiseBank] = None,
                 source_snr_db=(0.0, 20.0), dry_noise: bool = True, tempo=None, p_tempo: float = 1.0, pitch=None,
                 p_pitch: float = 1.0, stretch_hop: int = 256, stretch_search: int = 160, room_stats: bool = False,
                 motion=None, p_motion: float = 1.0, motion_hop_ms: float = 250.0, source_motion=None,
                 dynamics: Optional[DynamicsSampler] = None, dynamics_on: str = "noisy", noise: Optional[NoiseSampler] = None,
                 transmission: Optional["TransmissionSampler"] = None, transmission_on: str = "noisy",
                 suppressor: Optional["SuppressorSampler"] = None, suppressor_on: str = "noisy"):
        if sources is not None:
            given, counts = sources, "(low, high) whole numbers with 0 <= low <= high and 1 <= high <= 4"
            sources = _pair("sources", given, 0, 4, counts, "None or (low, high)", whole=True)
            if sources[1] < 1:
                raise ValueError(f"sources must be {counts}, got {given}")
            source_snr_db = _pair("source_snr_db", source_snr_db, -math.inf, math.inf, "(low, high) with low <= high", echo=True)
            if source_bank is not None and source_bank.device != engine.device:
                raise RuntimeError(f"source_bank is on {source_bank.device} but the engine is bound to {engine.device}")
        elif source_bank is not None:
            raise ValueError("source_bank given without sources")
        elif not dry_noise:
            raise ValueError("dry_noise=False needs sources: the batch would hold no noise at all")
        self.sources, self.source_snr_db, self.dry_noise = sources, source_snr_db, bool(dry_noise)
        self.source_bank = source_bank if source_bank is not None else noise_bank
        self.speed = speed = None if speed is None else _rate_pair("speed", speed)
        self.p_speed = _probability("p_speed", p_speed)
        self.speed_zeros, self.speed_rolloff = int(speed_zeros), float(speed_rolloff)       # Engine.warp judges them
        self.tempo = tempo = None if tempo is None else _rate_pair("tempo", tempo)
        if pitch is not None:
            pitch = _pair("pitch", pitch, -PITCH_RANGE, PITCH_RANGE, f"(low, high) semitones with {-PITCH_RANGE} <= low <= high "
                          f"<= {PITCH_RANGE}", "None or (low, high) in semitones", echo=True)
        self.pitch, self.p_tempo, self.p_pitch = pitch, _probability("p_tempo", p_tempo), _probability("p_pitch", p_pitch)
        for name, v, limits in (("stretch_hop", stretch_hop, STRETCH_HOP), ("stretch_search", stretch_search, STRETCH_SEARCH)):
            if not _whole_in(v, *limits):
                raise ValueError(f"{name} must be a whole number in [{limits[0]}, {limits[1]}], got {v}")
        self.stretch_hop, self.stretch_search = int(stretch_hop), int(stretch_search)
        self.last_stretch: Optional[StretchDraw] = None
        if tempo is not None or pitch is not None:
            (t_lo, t_hi), (f_lo, f_hi), (v_lo, v_hi) = self._ranges()
            if not (SPEED_RANGE[0] <= t_lo / f_hi and t_hi / f_lo <= SPEED_RANGE[1]):
                raise ValueError(f"tempo / pitch: the stretch rates, {t_lo / f_hi:.4g} .. {t_hi / f_lo:.4g}, must stay in "
                                 f"[{SPEED_RANGE[0]}, {SPEED_RANGE[1]}] (tempo = {tempo}, pitch = {pitch})")
            if not (SPEED_RANGE[0] <= v_lo * f_lo and v_hi * f_hi <= SPEED_RANGE[1]):
                raise ValueError(f"speed x pitch: the warp rates, {v_lo * f_lo:.4g} .. {v_hi * f_hi:.4g}, must stay in "
                                 f"[{SPEED_RANGE[0]}, {SPEED_RANGE[1]}] (speed = {speed}, pitch = {pitch})")
        if channel_on not in ("noisy", "both"):
            raise ValueError(f"channel_on must be 'noisy' or 'both', got {channel_on!r}")
        if channel is not None and not isinstance(channel, ChannelSampler):
            raise TypeError(f"channel must be a ChannelSampler or None, got {type(channel).__name__}")
        self.channel, self.channel_on = channel, channel_on
        if snr_on not in ("rms", "active"):
            raise ValueError(f"snr_on must be 'rms' or 'active', got {snr_on!r}")
        if level_db is not None:
            level_db = _pair("level_db", level_db, -math.inf, math.inf, "(low, high) with finite low <= high",
                             "None or (low, high) in dBFS", closed=False, echo=True)
        if (snr_on == "active" or level_db is not None) and not 8000 <= int(sample_rate) <= 192000:
            raise ValueError(f"the speech level is measured at 8000 .. 192000 Hz, got sample_rate = {sample_rate}")
        self.snr_on, self.level_db, self.last_level = snr_on, level_db, None
        self.snr_db = _pair("snr_db", snr_db, -math.inf, math.inf, "(low, high) with low <= high", form=None)
        self.p_reverb = _probability("p_reverb", p_reverb, as_given=True)
        if early_ms is not None and early_ms < 0:
            raise ValueError(f"early_ms must be >= 0 or None, got {early_ms}")
        for name, bank in (("noise_bank", noise_bank), ("rir_bank", rir_bank)):
            if bank is not None and bank.device != engine.device:
                raise RuntimeError(f"{name} is on {bank.device} but the engine is bound to {engine.device}")
        self.engine, self.noise_bank, self.peak, self.generator = engine, noise_bank, float(peak), generator
        self.n_rirs = len(rir_bank) if rir_bank is not None else 0
        self.rir_bank = rir_bank.with_identity() if rir_bank is not None and p_reverb < 1.0 else rir_bank
        self.early = -1 if early_ms is None else int(round(early_ms * sample_rate / 1000.0))
        self.last_draw: Optional[Draw] = None
        self.rooms, self.sample_rate = rooms, int(sample_rate)
        if not isinstance(room_stats, bool):
            raise TypeError(f"room_stats must be a bool, got {type(room_stats).__name__}")
        if room_stats and rooms is None and (rir_bank is None or rir_bank.stats is None):
            raise ValueError("room_stats=True needs rooms, or a rir_bank that has been measured (RirBank.measure)")
        self.room_stats, self.last_room_stats = room_stats, None
        self.rir_taps, self.n_images, self.last_bank = 0, None, None
        self.last_bands: Optional[torch.Tensor] = None      # rooms=RoomSampler(bands=n): the float64 [B, n, 7] table of the batch
        self.last_tail: Optional[TailDraw] = None           # rooms=RoomSampler(tail_ms=...): the batch's tail draw
        self.last_dirs = None                               # a directional RoomSampler: ((orient, pattern) of the talkers, of the sources)
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
        # ---- motion: judged last, so that every earlier error is what it was
        self.motion = None if motion is None else _speed_pair("motion", motion)
        self.source_motion = None if source_motion is None else _speed_pair("source_motion", source_motion)
        self.p_motion = _probability("p_motion", p_motion)
        if (self.motion is not None or self.source_motion is not None) and rooms is None:
            raise ValueError("motion / source_motion need rooms: a path is simulated, a rir_bank of fixed responses cannot move")
        if self.source_motion is not None and sources is None:
            raise ValueError("source_motion given without sources")
        self.motion_hop = 0                                 # H, the samples between waypoints
        if self.motion is not None or self.source_motion is not None:
            if isinstance(motion_hop_ms, bool) or not isinstance(motion_hop_ms, (int, float)) or not 0.0 < motion_hop_ms < math.inf \
                    or not 1 <= round(motion_hop_ms * sample_rate / 1000.0) <= SCENE_MAX_HOP:
                raise ValueError(f"motion_hop_ms must give a hop of 1 .. 2^30 samples, got {motion_hop_ms} ms at {sample_rate} Hz")
            self.motion_hop = int(round(motion_hop_ms * sample_rate / 1000.0))
        # ---- dynamics
        if dynamics_on not in ("noisy", "both"):
            raise ValueError(f"dynamics_on must be 'noisy' or 'both', got {dynamics_on!r}")
        if dynamics is not None and not isinstance(dynamics, DynamicsSampler):
            raise TypeError(f"dynamics must be a DynamicsSampler or None, got {type(dynamics).__name__}")
        self.dynamics, self.dynamics_on = dynamics, dynamics_on
        self.last_dynamics: Optional[torch.Tensor] = None   # dynamics=...: the float64 [B] largest gain reduction per row, dB
        # ---- synthetic noise: judged last, so that every earlier error is what it was
        if noise is not None and not isinstance(noise, NoiseSampler):
            raise TypeError(f"noise must be a NoiseSampler or None, got {type(noise).__name__}")
        if noise is not None and noise_bank is not None:
            raise ValueError("give either a noise_bank or noise=NoiseSampler(...), not both")
        if noise is None and noise_bank is None:
            raise ValueError("the mixer needs noise: give a noise_bank, or noise=NoiseSampler(...) to synthesize it")
        self.noise = noise
        self.last_noise: Optional[NoiseDraw] = None         # noise=...: the draw the batch's noise rows were made from
        self._noise_rows: Optional[torch.Tensor] = None     # noise=...: the persistent float32 [B, N] allocation behind noise_bank
        self._own_sources = source_bank is None             # sources take their point noises from the noise bank
        # ---- transmission: judged last, so that every earlier error is what it was
        if transmission_on not in ("noisy", "both"):
            raise ValueError(f"transmission_on must be 'noisy' or 'both', got {transmission_on!r}")
        if transmission is not None and not isinstance(transmission, TransmissionSampler):
            raise TypeError(f"transmission must be a TransmissionSampler or None, got {type(transmission).__name__}")
        if transmission is not None:                        # the packet length and Engine.transmit's defaults at this rate
            try:
                transmit_scalars(self.sample_rate, transmission.frame(self.sample_rate))
            except ValueError as e:
                raise ValueError(f"transmission at sample_rate = {sample_rate}: {e}") from None
        self.transmission, self.transmission_on = transmission, transmission_on
        self.last_transmission: Optional[TransmitInfo] = None
        # ---- suppressor: judged after the transmission, so that every earlier error is what it was
        if suppressor_on not in ("noisy", "both"):
            raise ValueError(f"suppressor_on must be 'noisy' or 'both', got {suppressor_on!r}")
        if suppressor is not None and not isinstance(suppressor, SuppressorSampler):
            raise TypeError(f"suppressor must be a SuppressorSampler or None, got {type(suppressor).__name__}")
        self.suppressor, self.suppressor_on = suppressor, suppressor_on
        self.last_suppression: Optional[SuppressDraw] = None    # suppressor=...: the table and n_fft the batch went through

    def waypoints(self, N: int) -> int:
        """P = 1 + ceil((N - 1) / H): the waypoints a batch of N samples needs; more than 64 is refused."""
        P = 1 + -(-(int(N) - 1) // self.motion_hop)
        if P > SCENE_MAX_WAYPOINTS:
            raise ValueError(f"a batch of {N} samples with a waypoint every {self.motion_hop} needs {P} waypoints; up to "
                             f"{SCENE_MAX_WAYPOINTS} are supported: raise motion_hop_ms")
        return P

    # ---- the draws: one helper per kind, each a fixed sequence of calls on the mixer's generator --------------------
    def _rand(self, *shape, dtype=torch.float64) -> torch.Tensor:
        return torch.rand(*shape, dtype=dtype, generator=self.generator, device=self.engine.device)

    def _randint(self, low: int, high: int, *shape) -> torch.Tensor:
        return torch.randint(low, high, shape, generator=self.generator, device=self.engine.device)

    def _draw_uniform(self, rng, *shape, dtype=torch.float64) -> torch.Tensor:
        """Uniform in rng = (lo, hi)."""
        lo, hi = rng
        return lo + (hi - lo) * self._rand(*shape, dtype=dtype)

    def _draw_rate(self, B: int, rng, p: float, semitones: bool = False) -> torch.Tensor:
        """Uniform in rng = (lo, hi), or exactly 1.0 with probability 1 - p, from ONE rand(B, 2); semitones=True: the
        factor 2^(x / 12) of such a draw, clamped to the host's own 2^(lo / 12), 2^(hi / 12): the bounds the batch length
        was worked out from."""
        lo, hi = rng
        u = self._rand(B, 2)
        x = lo + (hi - lo) * u[:, 0]
        if semitones:
            x, lo, hi = torch.exp2(x / 12.0), 2.0 ** (lo / 12.0), 2.0 ** (hi / 12.0)
        return torch.where(u[:, 1] < p, torch.clamp(x, lo, hi), torch.ones_like(x))       # (the sum may round past hi)

    def _draw_item(self, bank: NoiseBank, *shape):
        """An item of the bank and a uniform offset into it, per element: (start, length, offset), int64."""
        item = self._randint(0, len(bank), *shape)
        start, length = bank.start[item].contiguous(), bank.length[item].contiguous()
        return start, length, torch.minimum((self._rand(*shape) * length).to(torch.int64), length - 1)

    def _draw_dry(self, index: torch.Tensor, identity: int):
        """With probability 1 - p_reverb a row is dry and its index becomes `identity`: (index, the mask of the wet rows);
        at p_reverb = 1 nothing is drawn and the mask is None."""
        if self.p_reverb >= 1.0:
            return index, None
        wet = self._rand(index.size(0), dtype=torch.float32) < self.p_reverb
        return torch.where(wet, index, torch.full_like(index, identity)), wet

    def _draw_responses(self, B: int):
        """(rir_index, rir_len, the room table, the rooms' own n_taps) of the talkers; the rooms are the sampler's draw."""
        dev = self.engine.device
        if self.rir_bank is not None:
            index, _ = self._draw_dry(self._randint(0, self.n_rirs, B), self.n_rirs)
            return index.to(torch.int32), self.rir_bank.length[index].contiguous(), None, None
        if self.rooms is not None:
            table, taps = self.rooms.draw(B, self.rir_taps, self.sample_rate, device=dev)
            index, wet = self._draw_dry(torch.arange(B, dtype=torch.int32, device=dev), B)
            return index, taps if wet is None else torch.where(wet, taps, torch.ones_like(taps)), table, taps
        return None, None, None, None

    def _draw_sources(self, B: int, table: Optional[torch.Tensor], taps: Optional[torch.Tensor]):
        """The trailing fields of a SceneDraw; `table` and `taps` are the rooms of _draw_responses."""
        S = self.sources[1]
        n_src = self._randint(self.sources[0], S + 1, B).to(torch.int32)
        start, length, off = self._draw_item(self.source_bank, B, S)
        snr = self._draw_uniform(self.source_snr_db, B, S, dtype=torch.float32)
        index = rlen = rooms = None
        if self.rir_bank is not None:
            index = self._randint(0, self.n_rirs, B, S)
            index, rlen = index.to(torch.int32), self.rir_bank.length[index].contiguous()
        elif table is not None:
            rooms = self.rooms.draw_sources(table, S)
            index = self._bank_rows(B) + torch.arange(B * S, dtype=torch.int32, device=table.device).reshape(B, S)
            rlen = taps[:, None].expand(B, S).contiguous()
        return n_src, start, length, off, snr, index, rlen, rooms

    def _bank_rows(self, B: int, P: int = 1) -> int:
        """The rows of the simulated bank in front of the sources' responses: the talkers' (P per row when they move) and,
        with dry rows, the identity."""
        return B * P + (1 if self.p_reverb < 1.0 else 0)

    def draw(self, B: int):
        start, length, off = self._draw_item(self.noise_bank, B)
        snr = self._draw_uniform(self.snr_db, B, dtype=torch.float32)
        index, rlen, table, taps = self._draw_responses(B)
        level = None if self.level_db is None else self._draw_uniform(self.level_db, B)
        speed = None if self.speed is None else self._draw_rate(B, self.speed, self.p_speed)
        chan = None if self.channel is None else self.channel.draw(B, self.sample_rate, device=self.engine.device)
        drawn = Draw(start, length, off, snr, index, rlen, table, level, chan, speed)
        return drawn if self.sources is None else SceneDraw(*drawn, *self._draw_sources(B, table, taps))

    def _ranges(self):
        return _stretch_ranges(self.tempo, self.pitch, self.speed, self.p_tempo, self.p_pitch, self.p_speed)

    def stretch_len(self, L: int) -> int:
        """The batch length this mixer makes of clips of L samples (`stretch_len` with the mixer's ranges; `warp_len(L,
        hi)` with `speed` alone, L without any of the three)."""
        if self.tempo is None and self.pitch is None:
            return L if self.speed is None else warp_len(L, self.speed[1])
        return stretch_len(L, self.tempo, self.pitch, self.speed, self.p_tempo, self.p_pitch, self.p_speed)

    def draw_stretch(self, B: int, speed: Optional[torch.Tensor] = None) -> Optional[StretchDraw]:
        """The tempo and pitch draws of a batch (None when both are off), made after `draw`; `speed` is its Draw.speed."""
        if self.tempo is None and self.pitch is None:
            return None
        one = torch.ones(B, dtype=torch.float64, device=self.engine.device)
        t = one if self.tempo is None else self._draw_rate(B, self.tempo, self.p_tempo)
        f = one if self.pitch is None else self._draw_rate(B, self.pitch, self.p_pitch, semitones=True)
        warp = None
        if self.pitch is not None or speed is not None:
            warp = (f if speed is None else speed * f).contiguous()
        return StretchDraw(t, f, (t / f).contiguous(), warp)

    def draw_bands(self, d: Draw) -> Optional[torch.Tensor]:
        """The band table of a batch's rooms (None unless rooms=RoomSampler(bands=n)): RoomSampler.draw_bands of d.rooms,
        made after `draw` - the sources' draws included - so every other draw is what it is without bands.  Draw and
        SceneDraw keep their fields: the table of the last call stays readable as `mixer.last_bands`."""
        if self.rooms is None or self.rooms.bands is None:
            return None
        return self.rooms.draw_bands(d.rooms)

    def draw_tail(self, d: Draw) -> Optional[TailDraw]:
        """The diffuse tails of a batch's rooms (None unless rooms=RoomSampler(tail_ms=...)): RoomSampler.draw_tail of
        d.rooms and, with sources, d.src_rooms, made after `draw` and `draw_bands`; kept as `mixer.last_tail`."""
        if self.rooms is None or self.rooms.tail_ms is None:
            return None
        return self.rooms.draw_tail(d.rooms, self.sample_rate, getattr(d, "src_rooms", None))

    def draw_paths(self, d: Draw, N: int, tail: Optional[TailDraw] = None) -> Optional[_Paths]:
        """The walks of a batch of N samples (None unless `motion` or `source_motion`): RoomSampler.draw_path of d.rooms
        and then of d.src_rooms, made after `draw`, `draw_bands` and `draw_tail`, over the (P - 1) H samples the waypoints
        span.  A waypoint's n_taps is its row's - with `tail` its OWN junction - and 1 on a row drawn dry."""
        if self.motion is None and self.source_motion is None:
            return None
        P, fs = self.waypoints(N), self.sample_rate
        seconds = max(P - 1, 1) * self.motion_hop / float(fs)
        path = taps = src_path = src_taps = None
        if self.motion is not None:
            path = self.rooms.draw_path(d.rooms, P, seconds, speed=self.motion)
            taps = d.rir_len[:, None].expand(-1, P)
            if tail is not None:                                  # (d.rir_len is 1 on a dry row, else waypoint 0's junction)
                taps = torch.where(taps > 1, self.rooms._junction(path, tail.n_full[:, None], fs), taps)
            taps = taps.contiguous()
        if self.source_motion is not None:
            src_path = self.rooms.draw_path(d.src_rooms, P, seconds, speed=self.source_motion)
            src_taps = (d.src_rir_len[:, :, None].expand(-1, -1, P) if tail is None
                        else self.rooms._junction(src_path, tail.n_full[:, None, None], fs)).contiguous()
        return _Paths(P, path, taps, src_path, src_taps)

    def _draw_moving(self, B: int, paths: _Paths) -> torch.Tensor:
        """n_path: P with probability p_motion, else 1 - one rand(B) of the mixer's generator; all 1 without `motion`."""
        one = torch.ones(B, dtype=torch.int32, device=self.engine.device)
        if paths.path is None:
            return one
        return torch.where(self._rand(B, dtype=torch.float32) < self.p_motion, one * paths.P, one)

    def _path_draw(self, d: Draw, sim: RirBank, paths: _Paths, extended: bool) -> PathDraw:
        """`d` as a PathDraw: the [B, P] / [B, S, P] tables of Engine.scene_path over the simulated bank, a dry row on the
        identity in every column, whoever stands still on its one response in every column; extended: the lengths are
        those Engine.rir_tail left in the bank."""
        B, P, dev = d.rooms.size(0), paths.P, self.engine.device
        Pt = 1 if paths.path is None else P
        base = self._bank_rows(B, Pt)
        index = torch.arange(B * Pt, dtype=torch.int32, device=dev).reshape(B, Pt)
        if self.p_reverb < 1.0:
            index = torch.where((d.rir_index != B)[:, None], index, torch.full_like(index, B * Pt))
        rlen = sim.length[:B * Pt].reshape(B, Pt) if extended else (d.rir_len[:, None] if paths.path is None else paths.taps)
        out = PathDraw(*d)._replace(rir_index=index.expand(B, P).contiguous(), rir_len=rlen.expand(B, P).contiguous(), path=paths.path)
        if self.sources is None:
            return out
        S = self.sources[1]
        Ps = 1 if paths.src_path is None else P
        index = base + torch.arange(B * S * Ps, dtype=torch.int32, device=dev).reshape(B, S, Ps)
        rlen = sim.length[base:].reshape(B, S, Ps) if extended else (d.src_rir_len[:, :, None] if paths.src_path is None else paths.src_taps)
        return out._replace(src_rir_index=index.expand(B, S, P).contiguous(), src_rir_len=rlen.expand(B, S, P).contiguous(),
                            src_path=paths.src_path, src_n_path=torch.full((B, S), Ps, dtype=torch.int32, device=dev))

    def _extended(self, d: Draw, sim: RirBank) -> Draw:
        """`d` with the lengths Engine.rir_tail left in the simulated bank in place of the junctions that were drawn."""
        B = d.rooms.size(0)
        d = d._replace(rir_len=sim.length[:B].clone())
        if self.sources is None:
            return d
        return d._replace(src_rir_len=sim.length[self._bank_rows(B):].reshape(B, self.sources[1]).clone())

    def _simulate(self, d: Draw, bands: Optional[torch.Tensor] = None, tail: Optional[TailDraw] = None,
                  paths: Optional[_Paths] = None) -> RirBank:
        """The batch's responses, simulated into the persistent allocation (made anew only when its row count changes);
        with `bands` by Engine.rir_bands, a source using its room's band table; with `tail` each call stops at the rows'
        junctions and Engine.rir_tail adds the rest, a source from its own junction with its room's decay and a seed of
        its own.  With `paths` the same calls simulate every waypoint: Pt rows per talker, Ps per source, each with its
        room's bands, decay and whole length and its PATH's seed."""
        B, K = d.rooms.size(0), self.rir_taps
        Pt = 1 if paths is None or paths.path is None else paths.P
        Ps = 1 if paths is None or paths.src_path is None else paths.P
        talkers = B * Pt
        base = self._bank_rows(B, Pt)
        n_s = self.sources[1] if self.sources is not None else 0
        rows = base + B * n_s * Ps
        each = lambda t, n: t if n == 1 else t.repeat_interleave(n, dim=0)        # a row's value for each of its n responses
        if self.last_bank is None or self.last_bank.data.size(0) != rows:
            data = torch.zeros(rows, K, dtype=torch.float32, device=self.engine.device)
            length = torch.ones(rows, dtype=torch.int32, device=self.engine.device)
            if base > talkers:
                data[talkers, 0] = 1.0                            # the identity of the dry rows
            self.last_bank = RirBank(data, length)
        sim = self.last_bank
        # rir_len is the sampler's n_taps, or 1 for a dry row (whose response is then one tap that no row uses)
        filt = None if bands is None else self.rooms.filters(self.sample_rate, self.engine.device)

        def simulate(rooms, taps, out, table, dirs):
            orient, pattern = (None, None) if dirs is None else (dirs[0].reshape(-1, 6), dirs[1].reshape(rooms.size(0), -1, 2))
            if table is None:
                self.engine.rir(rooms, taps, K, self.n_images, fs=self.sample_rate, out=out, orient=orient, pattern=pattern)
            else:
                self.engine.rir_bands(rooms, table, taps, K, filt, self.n_images, fs=self.sample_rate, out=out, orient=orient,
                                      pattern=pattern)

        # a directional sampler: its draw_dirs of the talkers, then of the sources (whatever way those face), after every
        # other draw of the sampler; kept as `last_dirs`
        aimed = self.rooms.directional
        dirs = src_dirs = None

        def extend(out, n_full, decay, seed):                     # (a dry row's junction is 1: no window fits, it stays)
            self.engine.rir_tail(*out, n_full, decay, seed, filt, fs=self.sample_rate, window_ms=self.rooms.tail_window_ms)

        out = (sim.data[:talkers], sim.length[:talkers])
        if Pt == 1:
            dirs = self.rooms.draw_dirs(d.rooms) if aimed else None
            simulate(d.rooms, d.rir_len, out, bands, dirs)
        else:
            dirs = self.rooms.draw_dirs(paths.path, path=True) if aimed else None
            simulate(paths.path.reshape(talkers, 15), paths.taps.reshape(talkers), out, None if bands is None else each(bands, Pt), dirs)
        if tail is not None:
            extend(out, each(tail.n_full, Pt), each(tail.decay, Pt), each(tail.seed, Pt))
        if n_s:                                                   # the sources' responses: one call of B S (Ps) rows
            out = (sim.data[base:], sim.length[base:])
            if Ps == 1:
                rooms, taps = d.src_rooms, d.src_rir_len if tail is None else tail.src_junction
            else:
                rooms, taps = paths.src_path, paths.src_taps
            src_dirs = self.rooms.draw_dirs(rooms, path=Ps > 1, facing_deg=(0.0, 180.0)) if aimed else None
            simulate(rooms.reshape(B * n_s * Ps, 15), taps.reshape(B * n_s * Ps), out,
                     None if bands is None else bands.repeat_interleave(n_s * Ps, dim=0), src_dirs)
            if tail is not None:
                extend(out, tail.n_full.repeat_interleave(n_s * Ps), tail.decay.repeat_interleave(n_s * Ps, dim=0),
                       each(tail.src_seed.reshape(B * n_s), Ps))
        self.last_dirs = (dirs, src_dirs) if aimed else None
        return sim

    @staticmethod
    def level_gain(level, level_db: torch.Tensor) -> torch.Tensor:
        """The float32 [B] factor that takes rows measured as `level` (a SpeechLevel) to the active level `level_db`
        (float64 [B], dBFS): f32(sqrt(10^(level_db / 10) / active_ms)), and 1 where active_ms is not finite and > 0."""
        ok = torch.isfinite(level.active_ms) & (level.active_ms > 0)
        active = torch.where(ok, level.active_ms, torch.ones_like(level.active_ms))
        gain = torch.sqrt(torch.pow(10.0, level_db / 10.0) / active)
        return torch.where(ok, gain, torch.ones_like(gain)).to(torch.float32)

    def _synthesize(self, B: int, N: int) -> None:
        """noise=...: B fresh rows of N samples (NoiseBank.synthesize, one Engine.noise call) into the persistent allocation,
        overwritten in place, installed as `noise_bank` - and as `source_bank` where the sources share it."""
        if self._noise_rows is None or tuple(self._noise_rows.shape) != (B, N):
            self._noise_rows = torch.empty(B, N, dtype=torch.float32, device=self.engine.device)
        self.noise_bank = NoiseBank._synthesize(self.engine, self.noise, B, N, self.sample_rate, self._noise_rows)
        self.last_noise = self.noise_bank.draw
        if self._own_sources:
            self.source_bank = self.noise_bank

    def __call__(self, clean: torch.Tensor):
        B = clean.size(0)
        if self.noise is not None:                                # the batch's noise: made before every draw
            self._synthesize(B, self.stretch_len(clean.size(1)))
        d = self.last_draw = self.draw(B)
        bands = self.last_bands = self.draw_bands(d)
        tail = self.last_tail = self.draw_tail(d)
        moving = self.motion is not None or self.source_motion is not None
        paths = self.draw_paths(d, self.stretch_len(clean.size(1)), tail) if moving else None
        rir = self.rir_bank if self.rooms is None else self._simulate(d, bands, tail, paths)
        if paths is not None:                                     # the [B, P] tables over the simulated waypoints
            d = self.last_draw = self._path_draw(d, rir, paths, tail is not None)
        elif tail is not None:                                    # the batch is mixed with the extended responses
            d = self.last_draw = self._extended(d, rir)
        self.last_room_stats = self._room_stats(d, rir, bands)
        s = self.last_stretch = self.draw_stretch(B, d.speed)
        if paths is not None:                                     # who moves: the last draw of all
            d = self.last_draw = d._replace(n_path=self._draw_moving(B, paths))
        dyn = None if self.dynamics is None else self.dynamics.draw(B, self.sample_rate, device=self.engine.device)
        sup = None if self.suppressor is None else self.suppressor.draw(B, self.sample_rate, device=self.engine.device)
        # the link is the last draw of the call: _perturb, _level, _mix, _dynamics, _channel and _suppression below draw nothing (a
        # stage that does would have to draw above this line, or a sampler on the device's default generator would no longer come last)
        link = None if self.transmission is None else self.transmission.draw(
            B, -(-self.stretch_len(clean.size(1)) // self.transmission.frame(self.sample_rate)), device=self.engine.device)
        clean = self._perturb(d, s, clean)
        shift, clean = self._level(d, clean)
        noisy, target, info = self._mix(d, clean, rir, shift)
        if dyn is not None:
            d = self.last_draw = self._dynamics(d, dyn, noisy, target)
        self._channel(d, noisy, target)
        if sup is not None:
            self._suppression(sup, noisy, target)
        if link is not None:
            self._transmission(link, noisy, target)
        return target, noisy, info

    # ---- the stages of a call, in its order -------------------------------------------------------------------------
    def _room_stats(self, d: Draw, rir: Optional[RirBank], bands: Optional[torch.Tensor]) -> Optional[RirStats]:
        """What the talkers' responses of the batch measure as: measured (rooms) or gathered from the measured bank."""
        if not self.room_stats:
            return None
        if self.rooms is None:
            index = d.rir_index.to(torch.int64)
            return RirStats(*(t.index_select(0, index) for t in rir.stats))
        B = d.rooms.size(0)
        filt = None if bands is None else self.rooms.filters(self.sample_rate, self.engine.device)
        if isinstance(d, PathDraw):                               # a talker that moves is measured where it starts
            first = d.rir_index[:, 0].to(torch.int64)
            return self.engine.rir_stats(rir.data.index_select(0, first), d.rir_len[:, 0].contiguous(), filt, fs=self.sample_rate)
        return self.engine.rir_stats(rir.data[:B], rir.length[:B], filt, fs=self.sample_rate)

    def _perturb(self, d: Draw, s: Optional[StretchDraw], clean: torch.Tensor) -> torch.Tensor:
        """Tempo, pitch and speed: Engine.stretch and / or the ONE Engine.warp."""
        warp = lambda x, rate, N: self.engine.warp(x, rate, N, zeros=self.speed_zeros, rolloff=self.speed_rolloff)
        if s is None:
            return clean if d.speed is None else warp(clean, d.speed, warp_len(clean.size(1), self.speed[1]))
        (_, t_hi), (f_lo, f_hi), (_, v_hi) = self._ranges()
        N1 = warp_len(clean.size(1), t_hi / f_lo)
        clean = self.engine.stretch(clean, s.stretch_rate, N1, hop=self.stretch_hop, search=self.stretch_search)
        return clean if s.warp_rate is None else warp(clean, s.warp_rate, warp_len(N1, v_hi * f_hi))   # the speed stage's warp is this one

    def _level(self, d: Draw, clean: torch.Tensor):
        """The level measurement: (D, the batch at its drawn level), D the float64 [B] shift of snr_on="active" or None."""
        if self.snr_on != "active" and d.level_db is None:
            return None, clean
        lv = self.last_level = self.engine.speech_level(clean, fs=self.sample_rate)
        shift = None
        if self.snr_on == "active":
            ok = torch.isfinite(lv.activity) & (lv.activity > 0)
            shift = torch.where(ok, -10.0 * torch.log10(torch.where(ok, lv.activity, torch.ones_like(lv.activity))),
                                torch.zeros_like(lv.activity))
        if d.level_db is not None:
            clean = (clean * self.level_gain(lv, d.level_db)[:, None]).contiguous()
        return shift, clean

    def _mix(self, d: Draw, clean: torch.Tensor, rir: Optional[RirBank], shift: Optional[torch.Tensor]):
        """Engine.mix, or Engine.scene with sources: (noisy, target, info)."""
        def shifted(snr, by):
            return snr if by is None else (snr.to(torch.float64) - by).to(torch.float32).contiguous()
        snr = shifted(d.snr_db, shift)
        bank, early = (None, -1) if rir is None else (rir.data, self.early)
        if isinstance(d, PathDraw):
            src = (None,) * 9 if self.sources is None else (
                d.n_src, self.source_bank.data, d.src_start, d.src_len, d.src_off,
                shifted(d.src_snr_db, None if shift is None else shift[:, None]), d.src_n_path, d.src_rir_index, d.src_rir_len)
            dry = (self.noise_bank.data, d.noise_start, d.noise_len, d.noise_off, snr) if self.dry_noise else (None,) * 5
            return self.engine.scene_path(clean, self.motion_hop, d.n_path, bank, d.rir_index, d.rir_len, *dry, *src,
                                          peak=self.peak, early=early)
        if self.sources is None:
            return self.engine.mix(clean, self.noise_bank.data, d.noise_start, d.noise_len, d.noise_off, snr, bank,
                                   d.rir_index, d.rir_len, peak=self.peak, early=early)
        src_snr = shifted(d.src_snr_db, None if shift is None else shift[:, None])
        dry = (self.noise_bank.data, d.noise_start, d.noise_len, d.noise_off, snr) if self.dry_noise else (None,) * 5
        return self.engine.scene(clean, *dry, d.n_src, self.source_bank.data, d.src_start, d.src_len, d.src_off, src_snr,
                                 bank, d.rir_index, d.rir_len, d.src_rir_index, d.src_rir_len, peak=self.peak, early=early)

    def _dynamics(self, d: Draw, drawn: torch.Tensor, noisy: torch.Tensor, target: torch.Tensor):
        """The gain control, in place: on noisy, and with dynamics_on="both" the gain that noisy drives on target first;
        then the peak guard's rule once more, one factor for both.  Returns d with the table as `d.dynamics`."""
        table = self.dynamics.table(drawn, noisy)
        if self.dynamics_on == "both":
            self.engine.dynamics(target, table, key=noisy, out=target)
        _, _, self.last_dynamics = self.engine.dynamics(noisy, table, out=noisy, info=True)
        top = noisy.abs().amax(dim=1)
        scale = torch.where(top > self.peak, self.peak / top, torch.ones_like(top))[:, None]
        noisy.mul_(scale)
        target.mul_(scale)
        return _with_dynamics(d, table)

    def _channel(self, d: Draw, noisy: torch.Tensor, target: torch.Tensor) -> None:
        """The recording channel, in place: on noisy, and with channel_on="both" the shared sections on target."""
        if d.channel is None:
            return
        sos, n_sections, n_shared, clip_rel = d.channel
        self.engine.channel(noisy, sos, n_sections, self.channel_clip(clip_rel, noisy), out=noisy)
        if self.channel_on == "both":
            self.engine.channel(target, sos, n_shared, out=target)

    def _suppression(self, sup: SuppressDraw, noisy: torch.Tensor, target: torch.Tensor) -> None:
        """The device's noise suppressor, in place: on noisy, and with suppressor_on="both" the gains that noisy drives on
        target first."""
        if self.suppressor_on == "both":
            self.engine.suppress(target, sup.table, sup.n_fft, key=noisy, out=target)
        self.engine.suppress(noisy, sup.table, sup.n_fft, out=noisy)
        self.last_suppression = sup

    def _transmission(self, link: TransmitDraw, noisy: torch.Tensor, target: torch.Tensor) -> None:
        """The link, in place: on noisy, and with transmission_on="both" the same tables on target."""
        frame = self.transmission.frame(self.sample_rate)
        send = lambda x: self.engine.transmit(x, link.lost, frame, link.codec, link.plc, fs=self.sample_rate, out=x, info=True)
        target_lag = send(target)[2] if self.transmission_on == "both" else None
        _, status, lag = send(noisy)
        self.last_transmission = TransmitInfo(link, status, lag, target_lag)

    @staticmethod
    def channel_clip(clip_rel: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
        """The float64 [B] clipping level of Engine.channel for a drawn `clip_rel`: clip_rel x max |noisy| per row, and
        +inf (no limit) where clip_rel is +inf or the row is silent."""
        top = noisy.abs().amax(dim=1).to(torch.float64)
        on = torch.isfinite(clip_rel) & (top > 0)
        return torch.where(on, torch.where(on, clip_rel, torch.ones_like(clip_rel)) * top, torch.full_like(top, math.inf))


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
    With `DynamicMixer(speed=...)` the batch is `warp_len(L, hi)` samples long and the lengths are clamped to that; with
    `tempo=` / `pitch=` it is `mixer.stretch_len(L)` long, and they are clamped likewise.

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
            if self.mixer.speed is not None or self.mixer.last_stretch is not None:   # the batch is not as long as the clips it was made of
                length = torch.as_tensor(length).clamp(max=noisy.size(1))
            self._alive.append((clean, target, noisy, info, self.mixer.last_draw))
            self.last_info = info
            yield target, noisy, length
