"""Thin host wrapper over one libcmgan_hip handle.

PyTorch is used only for device memory and streams: every method takes CUDA (ROCm)
``torch.Tensor``s, passes their ``data_ptr()`` through the C ABI, and enqueues on
``torch.cuda.current_stream()``.  No arithmetic happens in Python.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import Config, KernelTime, Taps, check


def tensor_arg(t, name: str, dtype, device, shape_txt: Optional[str] = None, ok=None, contiguous: bool = True, error=None):
    """The one rule for a tensor argument (pure host code): a torch.Tensor (TypeError) of `dtype` (TypeError) on `device`
    (RuntimeError) for which `ok(t)` holds (ValueError naming `shape_txt`; None = any shape) and, unless told otherwise,
    contiguous (ValueError).  `error`: one exception type for every rule, for the arguments that have always raised
    ValueError whatever was wrong.  Returns t."""
    if not isinstance(t, torch.Tensor):
        kind, what = TypeError, f"expected a torch.Tensor, got {type(t).__name__}"
    elif t.dtype != dtype:
        kind, what = TypeError, f"expected {dtype}, got {t.dtype}".replace("torch.", "")
    elif t.device != device:
        kind, what = RuntimeError, f"tensor is on {t.device} but this Engine is bound to {device}"
    elif ok is not None and not ok(t):
        kind, what = ValueError, f"expected {shape_txt}, got {tuple(t.shape)}"
    elif contiguous and not t.is_contiguous():
        kind, what = ValueError, "must be contiguous"
    else:
        return t
    raise (error or kind)(f"{name}: {what}")


def native_call(eng, name: str, *args) -> None:
    """`name(handle, *args)` of eng.lib, checked.  A tensor goes as its device pointer, a parameter struct by reference,
    everything else as it is (None: a null pointer)."""
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
            for a in args]
    check(eng._h, getattr(eng.lib, name)(eng._h, *args))


def _on_device(fn):
    """Run an Engine method with the Engine's device current, so the launch stream, the workspace and the
    handle's own buffers all belong to the same GPU even when another device is current in the caller."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapper


_EPS = float(np.spacing(1.0))


class DeviceScores(NamedTuple):
    """Engine.metrics: float64 [B] device tensors; the first six are cmgan_amd.metrics.Scores' fields."""
    pesq: torch.Tensor
    csig: torch.Tensor
    cbak: torch.Tensor
    covl: torch.Tensor
    ssnr: torch.Tensor
    stoi: torch.Tensor
    wss: torch.Tensor
    llr: torch.Tensor
    snr: torch.Tensor


class FrameScores(NamedTuple):
    """Engine.metrics(per_frame=True): per-frame WSS, LLR and clipped segmental SNR, [B, frames] float64."""
    wss: torch.Tensor
    llr: torch.Tensor
    segsnr: torch.Tensor


class MixInfo(NamedTuple):
    """Engine.mix: float64 [B] device tensors - the noise gain, the peak scale and the powers of speech and noise, so the
    achieved SNR is 10 log10(Ps / (g^2 Pn)) without reading audio again."""
    g: torch.Tensor
    scale: torch.Tensor
    Ps: torch.Tensor
    Pn: torch.Tensor


MIX_MAX_TAPS = 65536          # longest RIR of cmgan_mix


def check_mix_args(device, clean, noise_bank, noise_start, noise_len, noise_off, snr_db, rir_bank=None, rir_index=None,
                   rir_len=None, peak: float = 0.99, early: int = -1):
    """Argument rules of Engine.mix: those of Engine.scene (check_scene_args) without located sources and with a dry
    noise that must be there.  Returns (B, L, R, Kmax)."""
    for name, t in (("noise_bank", noise_bank), ("noise_start", noise_start), ("noise_len", noise_len),
                    ("noise_off", noise_off), ("snr_db", snr_db)):
        if t is None:
            raise TypeError(f"{name}: expected a torch.Tensor, got NoneType")
    return check_scene_args(device, clean, noise_bank, noise_start, noise_len, noise_off, snr_db, rir_bank=rir_bank,
                            rir_index=rir_index, rir_len=rir_len, peak=peak, early=early)[:4]


class SceneInfo(NamedTuple):
    """Engine.scene: float64 device tensors - the gains g0 (dry noise), g_1 .. g_S and the powers Pn, P_1 .. P_S as
    [B, 1 + S] (0 in the columns beyond a row's own sources), the peak scale and the speech power as [B]."""
    g: torch.Tensor
    scale: torch.Tensor
    Ps: torch.Tensor
    P: torch.Tensor


SCENE_MAX_SOURCES = 4         # located sources per row (= cmgan_scene_max_sources())


def check_scene_args(device, clean, noise_bank=None, noise_start=None, noise_len=None, noise_off=None, snr_db=None,
                     n_src=None, src_bank=None, src_start=None, src_len=None, src_off=None, src_snr_db=None, rir_bank=None,
                     rir_index=None, rir_len=None, src_rir_index=None, src_rir_len=None, peak: float = 0.99, early: int = -1):
    """Argument rules of Engine.scene (shapes, dtypes, devices and host scalars; pure host code).  Returns (B, L, R, Kmax, S)."""
    tensor_arg(clean, "clean", torch.float32, device, "[B, L] with B, L >= 1",
               lambda t: t.dim() == 2 and t.size(0) >= 1 and t.size(1) >= 1)
    B, L = clean.shape
    if B > 65535:
        raise ValueError(f"clean: at most 65535 rows, got {B}")
    row = lambda t: tuple(t.shape) == (B,)
    dry = (("noise_start", noise_start, torch.int64), ("noise_len", noise_len, torch.int64),
           ("noise_off", noise_off, torch.int64), ("snr_db", snr_db, torch.float32))
    if noise_bank is None:
        given = [name for name, t, _ in dry if t is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} given without a noise_bank")
    else:
        tensor_arg(noise_bank, "noise_bank", torch.float32, device, "a flat bank of >= 1 samples",
                   lambda t: t.dim() == 1 and t.numel() >= 1)
        for name, t, dtype in dry:
            if t is None:
                raise ValueError(f"a noise_bank needs {name}")
            tensor_arg(t, name, dtype, device, f"[{B}]", row)
    src = (("src_start", src_start, torch.int64), ("src_len", src_len, torch.int64), ("src_off", src_off, torch.int64),
           ("src_snr_db", src_snr_db, torch.float32))
    S = 0
    if n_src is None:
        given = [name for name, t in (("src_bank", src_bank), *((n, t) for n, t, _ in src), ("src_rir_index", src_rir_index),
                                      ("src_rir_len", src_rir_len)) if t is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} given without n_src")
    else:
        tensor_arg(n_src, "n_src", torch.int32, device, f"[{B}]", row)
        if src_bank is None:
            raise ValueError("n_src needs a src_bank")
        tensor_arg(src_bank, "src_bank", torch.float32, device, "a flat bank of >= 1 samples",
                   lambda t: t.dim() == 1 and t.numel() >= 1)
        if src_start is None:
            raise ValueError("n_src needs src_start")
        tensor_arg(src_start, "src_start", torch.int64, device, f"[{B}, S] with 1 <= S <= {SCENE_MAX_SOURCES}",
                   lambda t: t.dim() == 2 and t.size(0) == B and 1 <= t.size(1) <= SCENE_MAX_SOURCES)
        S = int(src_start.size(1))
        table = lambda t: tuple(t.shape) == (B, S)
        for name, t, dtype in src[1:]:
            if t is None:
                raise ValueError(f"n_src needs {name}")
            tensor_arg(t, name, dtype, device, f"[{B}, {S}]", table)
    R, Kmax = 0, 0
    if rir_bank is None:
        given = [name for name, t in (("rir_index", rir_index), ("rir_len", rir_len), ("src_rir_index", src_rir_index),
                                      ("src_rir_len", src_rir_len)) if t is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} given without a rir_bank")
    else:
        tensor_arg(rir_bank, "rir_bank", torch.float32, device, "[R, Kmax] with R, Kmax >= 1",
                   lambda t: t.dim() == 2 and t.size(0) >= 1 and t.size(1) >= 1)
        R, Kmax = rir_bank.shape
        if Kmax > MIX_MAX_TAPS:
            raise ValueError(f"rir_bank: RIRs of up to {MIX_MAX_TAPS} taps are supported, got Kmax = {Kmax}")
        if rir_index is None or rir_len is None:
            raise ValueError("a rir_bank needs rir_index and rir_len")
        tensor_arg(rir_index, "rir_index", torch.int32, device, f"[{B}]", row)
        tensor_arg(rir_len, "rir_len", torch.int32, device, f"[{B}]", row)
        if S:
            if src_rir_index is None or src_rir_len is None:
                raise ValueError("a rir_bank with sources needs src_rir_index and src_rir_len")
            tensor_arg(src_rir_index, "src_rir_index", torch.int32, device, f"[{B}, {S}]", table)
            tensor_arg(src_rir_len, "src_rir_len", torch.int32, device, f"[{B}, {S}]", table)
    peak = float(peak)
    if not (peak > 0.0 and peak < float("inf")):
        raise ValueError(f"peak must be positive and finite, got {peak}")
    if int(early) != early or early < -1:
        raise ValueError(f"early must be -1 (dry target) or a sample count >= 0, got {early}")
    return B, L, R, Kmax, S


SCENE_MAX_WAYPOINTS = 64      # waypoint columns of a path (= cmgan_scene_max_waypoints())
SCENE_MAX_HOP = 2 ** 30       # largest hop between waypoints, in samples


def check_scene_path_args(device, clean, hop, n_path, rir_bank, rir_index, rir_len, noise_bank=None, noise_start=None,
                          noise_len=None, noise_off=None, snr_db=None, n_src=None, src_bank=None, src_start=None, src_len=None,
                          src_off=None, src_snr_db=None, src_n_path=None, src_rir_index=None, src_rir_len=None,
                          peak: float = 0.99, early: int = -1):
    """Argument rules of Engine.scene_path: those of Engine.scene (check_scene_args) for everything but the responses, a
    rir_bank that must be there, and the path tables.  Pure host code.  Returns (B, L, R, Kmax, S, P)."""
    # everything but the responses by the static rules
    B, L, _, _, S = check_scene_args(device, clean, noise_bank, noise_start, noise_len, noise_off, snr_db, n_src, src_bank,
                                     src_start, src_len, src_off, src_snr_db, peak=peak, early=early)
    if rir_bank is None:
        raise ValueError("a path needs a rir_bank")
    tensor_arg(rir_bank, "rir_bank", torch.float32, device, "[R, Kmax] with R, Kmax >= 1",
               lambda t: t.dim() == 2 and t.size(0) >= 1 and t.size(1) >= 1)
    R, Kmax = rir_bank.shape
    if Kmax > MIX_MAX_TAPS:
        raise ValueError(f"rir_bank: RIRs of up to {MIX_MAX_TAPS} taps are supported, got Kmax = {Kmax}")
    tensor_arg(rir_index, "rir_index", torch.int32, device, f"[{B}, P] with 1 <= P <= {SCENE_MAX_WAYPOINTS}",
               lambda t: t.dim() == 2 and t.size(0) == B and 1 <= t.size(1) <= SCENE_MAX_WAYPOINTS)
    P = int(rir_index.size(1))
    tensor_arg(rir_len, "rir_len", torch.int32, device, f"[{B}, {P}]", lambda t: tuple(t.shape) == (B, P))
    tensor_arg(n_path, "n_path", torch.int32, device, f"[{B}]", lambda t: tuple(t.shape) == (B,))
    if not _whole_in(hop, 1, SCENE_MAX_HOP):
        raise ValueError(f"hop must be a whole number of samples in [1, 2^30], got {hop}")
    if S:
        for name, t, shape in (("src_n_path", src_n_path, (B, S)), ("src_rir_index", src_rir_index, (B, S, P)),
                               ("src_rir_len", src_rir_len, (B, S, P))):
            if t is None:
                raise ValueError(f"a path with sources needs {name}")
            tensor_arg(t, name, torch.int32, device, f"{list(shape)}", lambda t, shape=shape: tuple(t.shape) == shape)
    else:
        given = [name for name, t in (("src_n_path", src_n_path), ("src_rir_index", src_rir_index), ("src_rir_len", src_rir_len))
                 if t is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} given without n_src")
    return B, L, R, Kmax, S, P


RIR_MAX_TAPS = 65536          # longest response of cmgan_rir (= MIX_MAX_TAPS: its output is a bank of cmgan_mix)
RIR_MAX_IMAGES = 255          # largest image index per axis
RIR_MAX_TW = 64               # largest half-width of the fractional-delay filter


def check_rir_args(device, rooms, n_taps, K, n_images, fs=16000, c: float = 343.0, tw: int = 40, out=None):
    """Argument rules of Engine.rir (shapes, dtypes, devices and host scalars; pure host code).  Returns (R, K, (Nx, Ny, Nz))."""
    tensor_arg(rooms, "rooms", torch.float64, device, "[R, 15] with R >= 1",
               lambda t: t.dim() == 2 and t.size(0) >= 1 and t.size(1) == 15)
    R = rooms.size(0)
    if R > 65535:
        raise ValueError(f"rooms: at most 65535 rows, got {R}")
    tensor_arg(n_taps, "n_taps", torch.int32, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    if int(K) != K or not 1 <= K <= RIR_MAX_TAPS:
        raise ValueError(f"K must be a tap count in [1, {RIR_MAX_TAPS}], got {K}")
    try:
        N = tuple(n_images)
    except TypeError:
        N = ()
    if len(N) != 3 or any(int(n) != n or not 0 <= n <= RIR_MAX_IMAGES for n in N):
        raise ValueError(f"n_images must be (Nx, Ny, Nz) with 0 <= N <= {RIR_MAX_IMAGES}, got {n_images}")
    N = tuple(int(n) for n in N)
    if 8 * (2 * N[0] + 1) * (2 * N[1] + 1) * (2 * N[2] + 1) >= 2 ** 31:
        raise ValueError(f"n_images: 8 (2Nx+1)(2Ny+1)(2Nz+1) must stay below 2^31, got {N}")
    if int(fs) != fs or fs < 1:
        raise ValueError(f"fs must be a positive sample rate, got {fs}")
    c = float(c)
    if not (c > 0.0 and c < float("inf")):
        raise ValueError(f"c must be positive and finite, got {c}")
    if not _whole_in(tw, 1, RIR_MAX_TW, allow_bool=True):
        raise ValueError(f"tw must be a half-width in [1, {RIR_MAX_TW}] samples, got {tw}")
    if out is not None:
        try:
            rir, length = out
        except (TypeError, ValueError):
            raise ValueError("out must be a pair (rir float32 [R, K], length int32 [R])") from None
        tensor_arg(rir, "out[0]", torch.float32, device, f"[{R}, {int(K)}]", lambda t: tuple(t.shape) == (R, int(K)))
        tensor_arg(length, "out[1]", torch.int32, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    return R, int(K), N


RIR_MAX_BANDS = 8             # most frequency bands of cmgan_rir_bands
RIR_MAX_FILTER = 1023         # longest filter of its filterbank (odd)


def check_rir_bands_args(device, rooms, bands, n_taps, K, filters, n_images, fs=16000, c: float = 343.0, tw: int = 40,
                         out=None):
    """Argument rules of Engine.rir_bands (shapes, dtypes, devices and host scalars; pure host code).  Returns
    (R, K, (Nx, Ny, Nz), NB, NF)."""
    R, K, N = check_rir_args(device, rooms, n_taps, K, n_images, fs, c, tw, out)
    tensor_arg(bands, "bands", torch.float64, device, f"[{R}, NB, 7] with 1 <= NB <= {RIR_MAX_BANDS}",
               lambda t: t.dim() == 3 and t.size(0) == R and 1 <= t.size(1) <= RIR_MAX_BANDS and t.size(2) == 7)
    NB = bands.size(1)
    tensor_arg(filters, "filters", torch.float64, device, f"[{NB}, NF] with NF odd in [1, {RIR_MAX_FILTER}]",
               lambda t: t.dim() == 2 and t.size(0) == NB and 1 <= t.size(1) <= RIR_MAX_FILTER and t.size(1) % 2 == 1)
    return R, K, N, NB, filters.size(1)


def check_rir_dir_args(device, R: int, NB: int, orient, pattern):
    """Argument rules of the directivity tables of Engine.rir (NB = 1) and Engine.rir_bands (pure host code): both or
    neither; orient float64 [R, 6], pattern float64 [R, NB, 2] ([R, 2] is accepted for [R, 1, 2]).  Returns (orient,
    pattern as [R, NB, 2]), or (None, None)."""
    if orient is None and pattern is None:
        return None, None
    if orient is None or pattern is None:
        raise ValueError(f"orient and pattern go together: {'orient' if orient is None else 'pattern'} is missing")
    tensor_arg(orient, "orient", torch.float64, device, f"[{R}, 6]", lambda t: tuple(t.shape) == (R, 6))
    tensor_arg(pattern, "pattern", torch.float64, device, f"[{R}, {NB}, 2]" + (f" or [{R}, 2]" if NB == 1 else ""),
               lambda t: tuple(t.shape) == (R, NB, 2) or (NB == 1 and tuple(t.shape) == (R, 2)))
    return orient, pattern.reshape(R, NB, 2)


RIR_STATS_COLUMNS = 10        # = cmgan_rir_stats_columns()
RIR_STATS_NONFINITE, RIR_STATS_ZERO, RIR_STATS_NO_EDT, RIR_STATS_NO_T20, RIR_STATS_NO_T30 = 1, 2, 4, 8, 16    # status bits


class RirStats(NamedTuple):
    """Engine.rir_stats: float64 [R, NB + 1] device tensors (column 0 broad-band, column 1 + b band b) - the response's
    energy, the index of its direct arrival, the direct-to-reverberant ratio, C50, C80 (dB), D50, the centre time Ts,
    EDT, T20 and T30 (seconds) - and the int32 status bits (RIR_STATS_*: 0 where everything could be measured)."""
    energy: torch.Tensor
    direct: torch.Tensor
    drr_db: torch.Tensor
    c50_db: torch.Tensor
    c80_db: torch.Tensor
    d50: torch.Tensor
    ts: torch.Tensor
    edt: torch.Tensor
    t20: torch.Tensor
    t30: torch.Tensor
    status: torch.Tensor


def check_rir_stats_args(device, rir, length=None, filters=None, fs=16000, direct_ms=2.5):
    """Argument rules of Engine.rir_stats (shapes, dtypes, devices and host scalars; pure host code).  Returns
    (R, K, NB, NF), NF = 1 without filters."""
    R, K = _row_batch(device, rir, RIR_MAX_TAPS, name="rir")
    if length is not None:
        tensor_arg(length, "length", torch.int32, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    NB, NF = 0, 1
    if filters is not None:
        tensor_arg(filters, "filters", torch.float64, device,
                   f"[NB, NF] with 1 <= NB <= {RIR_MAX_BANDS} and NF odd in [1, {RIR_MAX_FILTER}]",
                   lambda t: t.dim() == 2 and 1 <= t.size(0) <= RIR_MAX_BANDS and 1 <= t.size(1) <= RIR_MAX_FILTER
                   and t.size(1) % 2 == 1)
        NB, NF = filters.shape
    if isinstance(fs, bool) or int(fs) != fs or not 1 <= fs <= 2 ** 31 - 1:
        raise ValueError(f"fs must be a positive sample rate, got {fs}")
    direct_ms = float(direct_ms)
    if not 0.0 <= direct_ms < float("inf"):
        raise ValueError(f"direct_ms must be finite and >= 0, got {direct_ms}")
    return R, K, NB, NF


RIR_TAIL_MAX_WINDOW = 4096    # = cmgan_rir_tail_max_window(): the longest fit window in samples
RIR_TAIL_NOTHING, RIR_TAIL_WINDOW, RIR_TAIL_DECAY, RIR_TAIL_NONFINITE = 1, 2, 4, 8    # status bits


class RirTail(NamedTuple):
    """Engine.rir_tail: the fitted level A_b of every band (float64 [R, max(NB, 1)], 0 for a row left untouched) and the
    int32 [R] status (0, or the RIR_TAIL_* bits of the reasons a row was left untouched)."""
    gain: torch.Tensor
    status: torch.Tensor


def check_rir_tail_args(device, rir, length, n_taps, decay, seed, filters=None, fs=16000, window_ms=30.0):
    """Argument rules of Engine.rir_tail (shapes, dtypes, devices and host scalars; pure host code).  Returns
    (R, K, NB, NF, W): NB = 0 and NF = 1 without filters, W the window in samples."""
    R, K = _row_batch(device, rir, RIR_MAX_TAPS, name="rir")
    tensor_arg(length, "length", torch.int32, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    tensor_arg(n_taps, "n_taps", torch.int32, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    NB, NF = 0, 1
    if filters is not None:
        tensor_arg(filters, "filters", torch.float64, device,
                   f"[NB, NF] with 1 <= NB <= {RIR_MAX_BANDS} and NF odd in [1, {RIR_MAX_FILTER}]",
                   lambda t: t.dim() == 2 and 1 <= t.size(0) <= RIR_MAX_BANDS and 1 <= t.size(1) <= RIR_MAX_FILTER
                   and t.size(1) % 2 == 1)
        NB, NF = filters.shape
    NBp = max(NB, 1)
    tensor_arg(decay, "decay", torch.float64, device, f"[{R}, {NBp}]", lambda t: tuple(t.shape) == (R, NBp))
    tensor_arg(seed, "seed", torch.int64, device, f"[{R}]", lambda t: tuple(t.shape) == (R,))
    if isinstance(fs, bool) or int(fs) != fs or not 1 <= fs <= 2 ** 31 - 1:
        raise ValueError(f"fs must be a positive sample rate, got {fs}")
    window_ms = float(window_ms)
    W = int(window_ms * float(fs) / 1000.0 + 0.5) if 0.0 <= window_ms < float("inf") else 0      # round to nearest, halves up
    if not 1 <= W <= RIR_TAIL_MAX_WINDOW:
        raise ValueError(f"window_ms must give a window of 1 .. {RIR_TAIL_MAX_WINDOW} samples at fs = {fs}, got {window_ms}")
    return R, K, NB, NF, W


def _row_stride_ok(t, B: int, L: int) -> bool:
    return t.stride(1) == 1 and (B == 1 or t.stride(0) >= L)


def _row_batch(device, wav, max_L: Optional[int] = None, name: str = "wav"):
    """The rule for the batch of the augmentation calls: wav is a float32 [B, L] tensor of at most 65535 rows (of at most
    max_L samples), each contiguous and at least L from the next.  Returns (B, L)."""
    tensor_arg(wav, name, torch.float32, device, "[B, L] with B, L >= 1",
               lambda t: t.dim() == 2 and t.size(0) >= 1 and t.size(1) >= 1, contiguous=False)     # (its own stride rule below)
    B, L = wav.shape
    if B > 65535:
        raise ValueError(f"{name}: at most 65535 rows, got {B}")
    if max_L is not None and L > max_L:
        raise ValueError(f"{name}: rows of up to {max_L} samples are supported, got {L}")
    if not _row_stride_ok(wav, B, L):
        raise ValueError(f"{name}: rows must be contiguous and at least L apart, got strides {tuple(wav.stride())}")
    return B, L


def _whole_in(v, lo: int, hi: int, allow_bool: bool = False) -> bool:
    """Whether the host scalar v is a whole number in [lo, hi]; a bool is none unless allowed."""
    return (allow_bool or not isinstance(v, bool)) and int(v) == v and lo <= v <= hi


def _rate_batch(device, wav, rate, lengths):
    """The arguments Engine.warp and Engine.stretch share: the row batch, a float64 [B] rate and int32 [B] lengths or None.
    Returns (B, L)."""
    B, L = _row_batch(device, wav)
    row = lambda t: tuple(t.shape) == (B,)
    tensor_arg(rate, "rate", torch.float64, device, f"[{B}]", row)
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{B}]", row)
    return B, L


def _out_len(device, B: int, n_out, out):
    """The n_out / out pair of Engine.warp and Engine.stretch: n_out a length or None, out a float32 [B, N] tensor of such
    rows that agrees with it, or None.  Returns N, None when neither says it."""
    if n_out is not None and not _whole_in(n_out, 1, 2 ** 31 - 1):
        raise ValueError(f"n_out must be an output length in [1, 2^31 - 1] or None, got {n_out}")
    N = None if n_out is None else int(n_out)
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{B}, N]" if N is None else f"[{B}, {N}]",
                   lambda t: t.dim() == 2 and t.size(0) == B and t.size(1) >= 1 and (N is None or t.size(1) == N),
                   contiguous=False)
        N = int(out.size(1))
        if not _row_stride_ok(out, B, N):
            raise ValueError(f"out: rows must be contiguous and at least N apart, got strides {tuple(out.stride())}")
    return N


class SpeechLevel(NamedTuple):
    """Engine.speech_level: float64 [B] device tensors - the mean square of the row, the mean square over the time its
    talker is active (ITU-T P.56, method B) and their ratio, the fraction of the row that is active."""
    ms: torch.Tensor
    active_ms: torch.Tensor
    activity: torch.Tensor


LEVEL_FS = (8000, 192000)     # sample rates of cmgan_speech_level
LEVEL_TILE = 1024             # its samples per block (= cmgan_speech_level_tile())
LEVEL_MAX_L = 2 ** 31 - 1 - LEVEL_TILE


def level_workspace_bytes(B: int, L: int) -> int:
    """cmgan_speech_level_workspace_bytes: five float64 [B, tiles] planes, one float64 [B] and one int32 [B, tiles, 16],
    each rounded up to 256 bytes; 0 for a shape the kernels do not take."""
    if not (1 <= B <= 65535 and 1 <= L <= LEVEL_MAX_L):
        return 0
    up = lambda v: (v + 255) & ~255
    nt = (L + LEVEL_TILE - 1) // LEVEL_TILE
    return 5 * up(B * nt * 8) + up(B * 8) + up(B * nt * 16 * 4)


def check_level_args(device, wav, lengths=None, fs=16000):
    """Argument rules of Engine.speech_level (shapes, dtypes, devices and host scalars; pure host code).  Returns (B, L)."""
    B, L = _row_batch(device, wav, LEVEL_MAX_L)
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{B}]", lambda t: tuple(t.shape) == (B,))
    if not _whole_in(fs, *LEVEL_FS):
        raise ValueError(f"fs must be a sample rate in [{LEVEL_FS[0]}, {LEVEL_FS[1]}] Hz, got {fs}")
    return B, L


CHANNEL_TILE = 2048           # samples per block of cmgan_channel (= cmgan_channel_tile())
CHANNEL_MAX_SECTIONS = 8      # biquads per row (= cmgan_channel_max_sections())
CHANNEL_MAX_L = 2 ** 31 - 1 - CHANNEL_TILE


def channel_workspace_bytes(B: int, L: int, S: int) -> int:
    """cmgan_channel_workspace_bytes: with N = 2 x (S rounded up to 1, 2, 4 or 8), one int32 [B], one float64
    [B, 17, N, N] table of matrix powers and two float64 [B, tiles, N] planes, each rounded up to 256 bytes; 0 for a shape
    the kernels do not take."""
    if not (1 <= B <= 65535 and 1 <= L <= CHANNEL_MAX_L and 1 <= S <= CHANNEL_MAX_SECTIONS):
        return 0
    up = lambda v: (v + 255) & ~255
    N = 2 * next(p for p in (1, 2, 4, 8) if S <= p)
    nt = (L + CHANNEL_TILE - 1) // CHANNEL_TILE
    return up(B * 4) + up(B * 17 * N * N * 8) + 2 * up(B * nt * N * 8)


def check_channel_args(device, wav, sos, n_sections=None, clip=None, lengths=None, out=None):
    """Argument rules of Engine.channel (shapes, dtypes and devices; pure host code).  Returns (B, L, S)."""
    B, L = _row_batch(device, wav, CHANNEL_MAX_L)
    tensor_arg(sos, "sos", torch.float64, device, f"[{B}, S, 6] with 1 <= S <= {CHANNEL_MAX_SECTIONS}",
               lambda t: t.dim() == 3 and t.size(0) == B and 1 <= t.size(1) <= CHANNEL_MAX_SECTIONS and t.size(2) == 6)
    row = lambda t: tuple(t.shape) == (B,)
    if n_sections is not None:
        tensor_arg(n_sections, "n_sections", torch.int32, device, f"[{B}]", row)
    if clip is not None:
        tensor_arg(clip, "clip", torch.float64, device, f"[{B}]", row)
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{B}]", row)
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False)
        if not _row_stride_ok(out, B, L):
            raise ValueError(f"out: rows must be contiguous and at least L apart, got strides {tuple(out.stride())}")
        if out.data_ptr() == wav.data_ptr() and B > 1 and out.stride(0) != wav.stride(0):
            raise ValueError("out: in place needs the row stride of wav")
    return B, L, int(sos.size(1))


DYNAMICS_TILE = 64            # samples per tile of cmgan_dynamics: one wave (= cmgan_dynamics_tile())
DYNAMICS_BLOCK = 64 * DYNAMICS_TILE     # samples per block of its last pass: a tile per lane
DYNAMICS_MAX_L = 2 ** 31 - 1 - DYNAMICS_BLOCK


def dynamics_workspace_bytes(B: int, L: int) -> int:
    """cmgan_dynamics_workspace_bytes: a float64 [B, tiles, 65] plane of tile maps, a float64 [B, tiles] plane of entry
    states and a float64 [B, blocks] plane of peaks, each rounded up to 256 bytes; 0 for a shape the kernels do not take."""
    if not (1 <= B <= 65535 and 1 <= L <= DYNAMICS_MAX_L):
        return 0
    up = lambda v: (v + 255) & ~255
    nt = (L + DYNAMICS_TILE - 1) // DYNAMICS_TILE
    nb = (L + DYNAMICS_BLOCK - 1) // DYNAMICS_BLOCK
    return up(B * nt * (DYNAMICS_TILE + 1) * 8) + up(B * nt * 8) + up(B * nb * 8)


def _overlap(a: torch.Tensor, b: torch.Tensor, B: int, L: int) -> bool:
    """Whether the spans of two float32 [B, L] row batches intersect."""
    span = lambda t: (t.data_ptr(), t.data_ptr() + 4 * ((B - 1) * (t.stride(0) if B > 1 else L) + L))
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def check_dynamics_args(device, wav, dyn, key=None, lengths=None, out=None):
    """Argument rules of Engine.dynamics (shapes, dtypes, devices and overlaps; pure host code).  Returns (B, L)."""
    B, L = _row_batch(device, wav, DYNAMICS_MAX_L)
    tensor_arg(dyn, "dyn", torch.float64, device, f"[{B}, 6]", lambda t: tuple(t.shape) == (B, 6))
    if key is not None:
        tensor_arg(key, "key", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False)
        if not _row_stride_ok(key, B, L):
            raise ValueError(f"key: rows must be contiguous and at least L apart, got strides {tuple(key.stride())}")
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{B}]", lambda t: tuple(t.shape) == (B,))
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False)
        if not _row_stride_ok(out, B, L):
            raise ValueError(f"out: rows must be contiguous and at least L apart, got strides {tuple(out.stride())}")
        for name, t in (("wav", wav), ("key", key)):
            if t is None:
                continue
            same = out.data_ptr() == t.data_ptr() and (B == 1 or out.stride(0) == t.stride(0))
            if not same and _overlap(out, t, B, L):
                raise ValueError(f"out: overlaps {name}; only out = {name} itself (in place, the same row stride) is allowed")
    return B, L


NOISE_TILE = 256              # outputs per block of cmgan_noise (= cmgan_noise_tile())
NOISE_MAX_FILTER = 1023       # taps of a row's colouring filter (= cmgan_noise_max_filter())
NOISE_MAX_TONES = 8           # tones per row (= cmgan_noise_max_tones())
NOISE_MAX_POINTS = 4096       # envelope points per row (= cmgan_noise_max_points())
NOISE_MAX_N = 2 ** 31 - 1 - NOISE_TILE
NOISE_MAX_INDEX = 2 ** 40     # start + n may not exceed it


def noise_workspace_bytes(N: int) -> int:
    """cmgan_noise_workspace_bytes: one int32 [N] of verdicts, rounded up to 256 bytes; 0 for an N the kernels do not take."""
    return (N * 4 + 255) & ~255 if 1 <= N <= 65535 else 0


def check_noise_args(device, seed, fir, n, lengths=None, start=None, env=None, env_hop=None, tones=None, n_tones=None,
                     impulse=None, out=None):
    """Argument rules of Engine.noise (shapes, dtypes, devices and host scalars; pure host code).  Returns (N, K, NF, P, H,
    M): P = H = 0 without an envelope, M = 0 without tones."""
    tensor_arg(seed, "seed", torch.int64, device, "[N] with 1 <= N <= 65535", lambda t: t.dim() == 1 and 1 <= t.size(0) <= 65535)
    N = int(seed.size(0))
    tensor_arg(fir, "fir", torch.float64, device, f"[{N}, NF] with 1 <= NF <= {NOISE_MAX_FILTER}",
               lambda t: t.dim() == 2 and t.size(0) == N and 1 <= t.size(1) <= NOISE_MAX_FILTER)
    if not _whole_in(n, 0, NOISE_MAX_N):
        raise ValueError(f"n must be a length in [0, 2^31 - 1 - {NOISE_TILE}], got {n}")
    K = int(n)
    row = lambda t: tuple(t.shape) == (N,)
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{N}]", row)
    if start is not None:
        tensor_arg(start, "start", torch.int64, device, f"[{N}]", row)
    P = H = 0
    if env is not None:
        tensor_arg(env, "env", torch.float64, device, f"[{N}, P] with 1 <= P <= {NOISE_MAX_POINTS}",
                   lambda t: t.dim() == 2 and t.size(0) == N and 1 <= t.size(1) <= NOISE_MAX_POINTS)
        if env_hop is None or not _whole_in(env_hop, 1, 2 ** 31 - 1):
            raise ValueError(f"env_hop must be the samples between two points of env, a whole number in [1, 2^31 - 1], got {env_hop}")
        P, H = int(env.size(1)), int(env_hop)
    elif env_hop is not None:
        raise ValueError("env_hop given without env")
    M = 0
    if tones is not None:
        tensor_arg(tones, "tones", torch.float64, device, f"[{N}, M, 3] with 0 <= M <= {NOISE_MAX_TONES}",
                   lambda t: t.dim() == 3 and t.size(0) == N and t.size(1) <= NOISE_MAX_TONES and t.size(2) == 3)
        M = int(tones.size(1))
        if n_tones is not None:
            tensor_arg(n_tones, "n_tones", torch.int32, device, f"[{N}]", row)
    elif n_tones is not None:
        raise ValueError("n_tones given without tones")
    if impulse is not None:
        tensor_arg(impulse, "impulse", torch.float64, device, f"[{N}, 2]", lambda t: tuple(t.shape) == (N, 2))
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{N}, {K}]", lambda t: tuple(t.shape) == (N, K), contiguous=False)
        if K > 0 and not _row_stride_ok(out, N, K):
            raise ValueError(f"out: rows must be contiguous and at least n apart, got strides {tuple(out.stride())}")
    return N, K, int(fir.size(1)), P, H, M


WARP_TILE = 256               # outputs per block of cmgan_warp (= cmgan_warp_tile())
WARP_MAX_RATE = 4.0           # rates in [1 / 4, 4] (= cmgan_warp_max_rate())
WARP_ZEROS = (4, 64)          # zero crossings on either side of the filter's centre (64 = cmgan_warp_max_zeros())
WARP_ROLLOFF = (0.5, 1.0)     # the cutoff as a fraction of the lower Nyquist rate


def check_warp_args(device, wav, rate, n_out=None, lengths=None, zeros=24, rolloff=0.95, out=None):
    """Argument rules of Engine.warp (shapes, dtypes, devices and host scalars; pure host code).  Returns (B, L, N); N is
    None when neither n_out nor out says it (Engine.warp then takes cmgan_warp_out_len(L, 1 / 4))."""
    B, L = _rate_batch(device, wav, rate, lengths)
    if not _whole_in(zeros, *WARP_ZEROS):
        raise ValueError(f"zeros must be a whole number in [{WARP_ZEROS[0]}, {WARP_ZEROS[1]}], got {zeros}")
    if isinstance(rolloff, bool) or not WARP_ROLLOFF[0] <= float(rolloff) <= WARP_ROLLOFF[1]:
        raise ValueError(f"rolloff must lie in [{WARP_ROLLOFF[0]}, {WARP_ROLLOFF[1]}], got {rolloff}")
    return B, L, _out_len(device, B, n_out, out)


STRETCH_HOP = (16, 1024)      # samples per frame of cmgan_stretch (1024 = cmgan_stretch_max_hop())
STRETCH_SEARCH = (0, 1024)    # its search range on either side, in samples (1024 = cmgan_stretch_max_search())
PITCH_FACTOR = (0.5, 2.0)     # frequency ratios of Engine.pitch_shift: an octave either way


def check_stretch_args(device, wav, rate, n_out=None, lengths=None, hop=256, search=160, out=None):
    """Argument rules of Engine.stretch (shapes, dtypes, devices and host scalars; pure host code).  Returns (B, L, N); N
    is None when neither n_out nor out says it (Engine.stretch then takes cmgan_warp_out_len(L, 1 / 4))."""
    B, L = _rate_batch(device, wav, rate, lengths)
    if not _whole_in(hop, *STRETCH_HOP):
        raise ValueError(f"hop must be a whole number in [{STRETCH_HOP[0]}, {STRETCH_HOP[1]}], got {hop}")
    if not _whole_in(search, *STRETCH_SEARCH):
        raise ValueError(f"search must be a whole number in [{STRETCH_SEARCH[0]}, {STRETCH_SEARCH[1]}], got {search}")
    return B, L, _out_len(device, B, n_out, out)


def check_pitch_args(device, wav, factor, n_out=None, hop=256, search=160, zeros=24, rolloff=0.95):
    """Argument rules of Engine.pitch_shift, all judged before its first launch: those of Engine.stretch and Engine.warp,
    with `factor` a float64 [B] device tensor (its VALUES are judged on the device: a row outside [1/2, 2] comes out as
    zeros).  Returns (B, L)."""
    B, L = _row_batch(device, wav)
    tensor_arg(factor, "factor", torch.float64, device, f"[{B}]", lambda t: tuple(t.shape) == (B,))
    check_stretch_args(device, wav, factor, None, None, hop, search)
    check_warp_args(device, wav, factor, n_out, None, zeros, rolloff)
    return B, L


TRANSMIT_FRAME = (16, 4096)   # samples per frame of cmgan_transmit
TRANSMIT_LAG = (16, 1024)     # the lags its concealment may search (1024 = cmgan_transmit_max_lag())
TRANSMIT_WINDOW = (16, 1024)  # its matching window (1024 = cmgan_transmit_max_window())
TRANSMIT_CODECS = {"none": 0, "pcm16": 1, "ulaw": 2, "alaw": 3}    # the values of Engine.transmit's codec table


def transmit_scalars(fs=16000, frame=None, pmin=None, pmax=None, window=None, fade=None):
    """The host values of Engine.transmit with the defaults filled in from fs - frame fs / 50, pmin fs / 200, pmax 3 fs /
    200, window fs / 50, fade fs / 100 - as (frame, pmin, pmax, window, fade); a ValueError names what is out of range."""
    if not _whole_in(fs, 1, 2 ** 31 - 1):
        raise ValueError(f"fs must be a sample rate (a whole number >= 1), got {fs}")
    fs = int(fs)
    given = {"frame": (frame, fs // 50, TRANSMIT_FRAME), "pmin": (pmin, fs // 200, TRANSMIT_LAG),
             "pmax": (pmax, 3 * fs // 200, TRANSMIT_LAG), "window": (window, fs // 50, TRANSMIT_WINDOW),
             "fade": (fade, fs // 100, (1, 2 ** 31 - 1))}
    val = {}
    for name, (v, default, (lo, hi)) in given.items():
        note = "" if v is not None else f" (the default at fs = {fs})"
        v = default if v is None else v
        if not _whole_in(v, lo, hi):
            raise ValueError(f"{name} must be a whole number in [{lo}, {hi}], got {v}{note}")
        val[name] = int(v)
    if val["pmin"] > val["pmax"]:
        raise ValueError(f"pmin must not exceed pmax, got pmin = {val['pmin']}, pmax = {val['pmax']}")
    return val["frame"], val["pmin"], val["pmax"], val["window"], val["fade"]


def check_transmit_args(device, wav, lost, frame=None, codec=None, plc=None, lengths=None, fs=16000, pmin=None, pmax=None,
                        window=None, fade=None, out=None):
    """Argument rules of Engine.transmit (shapes, dtypes, devices and host scalars; pure host code): every error is a
    ValueError that names the argument.  Returns (B, L, frame, pmin, pmax, window, fade), the host values as
    `transmit_scalars` fills them in."""
    try:
        B, L = _row_batch(device, wav)
    except (TypeError, RuntimeError) as e:
        raise ValueError(str(e)) from None
    F, pmin, pmax, W, A = transmit_scalars(fs, frame, pmin, pmax, window, fade)
    K = -(-L // F)
    tensor_arg(lost, "lost", torch.uint8, device, f"[{B}, n_frames] with n_frames >= ceil(L / frame) = {K}",
               lambda t: t.dim() == 2 and t.size(0) == B and t.size(1) >= K, contiguous=False, error=ValueError)
    if not _row_stride_ok(lost, B, lost.size(1)):
        raise ValueError(f"lost: rows must be contiguous and at least n_frames apart, got strides {tuple(lost.stride())}")
    row = lambda t: tuple(t.shape) == (B,)
    for name, t in (("codec", codec), ("plc", plc), ("lengths", lengths)):
        if t is not None:
            tensor_arg(t, name, torch.int32, device, f"[{B}]", row, error=ValueError)
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False,
                   error=ValueError)
        if not _row_stride_ok(out, B, L):
            raise ValueError(f"out: rows must be contiguous and at least L apart, got strides {tuple(out.stride())}")
        same = out.data_ptr() == wav.data_ptr() and (B == 1 or out.stride(0) == wav.stride(0))
        if not same and _overlap(out, wav, B, L):
            raise ValueError("out: overlaps wav; only out = wav itself (in place, the same row stride) is allowed")
    return B, L, F, pmin, pmax, W, A


SUPPRESS_N_FFT = (256, 512, 1024)      # the transform sizes of cmgan_suppress
SUPPRESS_MAX_WINDOW = 128              # frames of its minimum search (= cmgan_suppress_max_window())
SUPPRESS_MAX_L = 2 ** 31 - 1 - 2048
SUPPRESS_RULES = {"off": 0, "wiener": 1, "specsub": 2, "logmmse": 3}    # column 0 of Engine.suppress's table


def suppress_frames(L: int, n_fft: int) -> int:
    """T = ceil(L / h) + 1 with h = n_fft / 2: the frames of an L-sample batch, the middle axis of Engine.suppress's gains."""
    h = n_fft // 2
    return -(-L // h) + 1


def suppress_workspace_bytes(B: int, L: int, n_fft: int) -> int:
    """cmgan_suppress_workspace_bytes: a complex128 [B, T, F] plane of spectra and a float64 [B, T, F] plane of periodograms
    and gains (T = suppress_frames(L, n_fft), F = n_fft / 2 + 1), each rounded up to 256 bytes; 0 for a shape the kernels do
    not take."""
    if not (1 <= B <= 65535 and 1 <= L <= SUPPRESS_MAX_L and n_fft in SUPPRESS_N_FFT):
        return 0
    up = lambda v: (v + 255) & ~255
    cells = B * suppress_frames(L, n_fft) * (n_fft // 2 + 1)
    return up(cells * 16) + up(cells * 8)


def check_suppress_args(device, wav, table, n_fft=512, lengths=None, key=None, out=None):
    """Argument rules of Engine.suppress (shapes, dtypes, devices, overlaps and n_fft; pure host code).  Returns (B, L)."""
    if isinstance(n_fft, bool) or n_fft not in SUPPRESS_N_FFT:
        raise ValueError(f"n_fft must be one of {SUPPRESS_N_FFT}, got {n_fft}")
    B, L = _row_batch(device, wav, SUPPRESS_MAX_L)
    tensor_arg(table, "table", torch.float64, device, f"[{B}, 7]", lambda t: tuple(t.shape) == (B, 7))
    if key is not None:
        tensor_arg(key, "key", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False)
        if not _row_stride_ok(key, B, L):
            raise ValueError(f"key: rows must be contiguous and at least L apart, got strides {tuple(key.stride())}")
    if lengths is not None:
        tensor_arg(lengths, "lengths", torch.int32, device, f"[{B}]", lambda t: tuple(t.shape) == (B,))
    if out is not None:
        tensor_arg(out, "out", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L), contiguous=False)
        if not _row_stride_ok(out, B, L):
            raise ValueError(f"out: rows must be contiguous and at least L apart, got strides {tuple(out.stride())}")
        for name, t in (("wav", wav), ("key", key)):
            if t is None:
                continue
            same = out.data_ptr() == t.data_ptr() and (B == 1 or out.stride(0) == t.stride(0))
            if not same and _overlap(out, t, B, L):
                raise ValueError(f"out: overlaps {name}; only out = {name} itself (in place, the same row stride) is allowed")
    return B, L


AUX_N_FFT = (256, 512, 1024, 2048)      # the window lengths of Engine.aux_loss (hop = n / 4)
AUX_MAX_RESOLUTIONS = 4
AUX_MAX_L = 2 ** 31 - 1 - 4096


class AuxLossOut(NamedTuple):
    """Engine.aux_loss: device tensors, nothing copied to the host."""
    total: torch.Tensor              # float32 [3]: A, its multi-resolution part, its SI-SDR part
    rows: torch.Tensor               # float64 [B, 2 R + 1]: (sc, lm) per resolution in n_ffts' order, then SI-SDR in dB
    grad: Optional[torch.Tensor]     # float32 [B, L] = dA / d est, or None (grad=False)


def check_aux_settings(n_ffts, w_mr, w_si):
    """The settings of Engine.aux_loss / training.AuxLoss (pure host code): 1 .. 4 distinct window lengths from AUX_N_FFT,
    two finite weights >= 0.  Returns (tuple of ints, float, float)."""
    try:
        res = tuple(n_ffts)
    except TypeError:
        raise TypeError(f"n_ffts: expected a sequence of window lengths, got {type(n_ffts).__name__}") from None
    if not 1 <= len(res) <= AUX_MAX_RESOLUTIONS:
        raise ValueError(f"n_ffts: need 1 to {AUX_MAX_RESOLUTIONS} resolutions, got {len(res)}")
    for n in res:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) not in AUX_N_FFT:
            raise ValueError(f"n_ffts: a resolution must be one of {AUX_N_FFT}, got {n!r}")
    res = tuple(int(n) for n in res)
    if len(set(res)) != len(res):
        raise ValueError(f"n_ffts: the resolutions must be distinct, got {res}")
    out = []
    for name, w in (("w_mr", w_mr), ("w_si", w_si)):
        if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name}: expected a number, got {type(w).__name__}")
        if not (np.isfinite(w) and w >= 0):
            raise ValueError(f"{name}: must be finite and >= 0, got {w}")
        out.append(float(w))
    return res, out[0], out[1]


def aux_loss_workspace_bytes(B: int, L: int, n_ffts) -> int:
    """cmgan_aux_loss_workspace_bytes: per resolution (T = 1 + L // (n / 4) frames of F = n / 2 + 1 bins) a complex128 and a
    float64 [B, T, F] plane and float64 [B, T, 3] partial sums, then float64 [B, ceil(L / 4096), 5], [B, 4, 2] and [B, 4];
    each rounded up to 256 bytes.  0 for arguments the kernels do not take."""
    try:
        res, _, _ = check_aux_settings(n_ffts, 0.0, 0.0)
    except (TypeError, ValueError):
        return 0
    if not (1 <= B <= 65535 and max(res) // 2 < L <= AUX_MAX_L):
        return 0
    up = lambda v: (v + 255) & ~255
    total = 0
    for n in res:
        T, F = 1 + L // (n // 4), n // 2 + 1
        total += up(B * T * F * 16) + up(B * T * F * 8) + up(B * T * 3 * 8)
    return total + up(B * (-(-L // 4096)) * 5 * 8) + up(B * 4 * 2 * 8) + up(B * 4 * 8)


def check_aux_loss_args(device, est, ref, n_ffts=(512, 1024, 2048), w_mr=1.0, w_si=0.0):
    """Argument rules of Engine.aux_loss (pure host code).  Returns (B, L, n_ffts, w_mr, w_si)."""
    res, w_mr, w_si = check_aux_settings(n_ffts, w_mr, w_si)
    tensor_arg(est, "est", torch.float32, device, "[B, L]", lambda t: t.dim() == 2 and t.size(0) >= 1)
    B, L = (int(v) for v in est.shape)
    tensor_arg(ref, "ref", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L))
    if B > 65535:
        raise ValueError(f"est: at most 65535 rows, got {B}")
    if not max(res) // 2 < L <= AUX_MAX_L:
        raise ValueError(f"est: rows must hold more than {max(res) // 2} samples (reflect padding of the {max(res)}-point "
                         f"window) and at most {AUX_MAX_L}, got {L}")
    return B, L, res, w_mr, w_si


STOI_MIN_L = 6554                       # the shortest 16 kHz row with 31 frames at 10 kHz (one 30-frame window)
STOI_MAX_L = (2 ** 31 - 1) // 5 - 4096


class StoiLossOut(NamedTuple):
    """Engine.stoi_loss: device tensors, nothing copied to the host."""
    total: torch.Tensor              # float32 [1]: A = sum_b -(weight / B) STOI_b over the rows without a status
    rows: torch.Tensor               # float64 [B, 2]: (STOI or ESTOI, kept frames); the value is NaN where the row has a status
    status: torch.Tensor             # int32 [B]: bit 0 = fewer than 31 kept frames, bit 1 = the value is not finite
    grad: Optional[torch.Tensor]     # float32 [B, L] = dA / d est (exact zeros on a row with a status), or None (grad=False)


def check_stoi_settings(w_stoi, extended):
    """The settings of Engine.stoi_loss / training.AuxLoss (pure host code): a finite weight >= 0 and a bool.  Returns
    (float, bool)."""
    if isinstance(w_stoi, bool) or not isinstance(w_stoi, (int, float, np.integer, np.floating)):
        raise TypeError(f"w_stoi: expected a number, got {type(w_stoi).__name__}")
    if not (np.isfinite(w_stoi) and w_stoi >= 0):
        raise ValueError(f"w_stoi: must be finite and >= 0, got {w_stoi}")
    if not isinstance(extended, (bool, np.bool_)):
        raise TypeError(f"stoi_extended: expected a bool, got {type(extended).__name__}")
    return float(w_stoi), bool(extended)


def stoi_frames(L: int) -> int:
    """Frames of 256 samples (hop 128) that a 16 kHz row of L samples has at 10 kHz, before the silent ones are removed."""
    n10 = -(-5 * L // 8)
    return -(-(n10 - 256) // 128) if n10 > 256 else 0


def check_stoi_loss_args(device, est, ref, weight=1.0, extended=False):
    """Argument rules of Engine.stoi_loss (pure host code).  Returns (B, L, weight, extended)."""
    weight, extended = check_stoi_settings(weight, extended)
    tensor_arg(est, "est", torch.float32, device, "[B, L]", lambda t: t.dim() == 2 and t.size(0) >= 1)
    B, L = (int(v) for v in est.shape)
    tensor_arg(ref, "ref", torch.float32, device, f"[{B}, {L}]", lambda t: tuple(t.shape) == (B, L))
    if B > 65535:
        raise ValueError(f"est: at most 65535 rows, got {B}")
    if not STOI_MIN_L <= L <= STOI_MAX_L:
        raise ValueError(f"est: rows must hold at least {STOI_MIN_L} samples (31 frames at 10 kHz, one 30-frame window) and at "
                         f"most {STOI_MAX_L}, got {L}")
    return B, L, weight, extended


PHASE_MAX_T = 1000000
PHASE_MAX_F = 1024


class PhaseLossOut(NamedTuple):
    """Engine.phase_loss: device tensors, nothing copied to the host."""
    total: torch.Tensor              # float32 [4]: (A, its IP part, its GD part, its IAF part), A = sum_b sum_i (w_i / B) value_i
    rows: torch.Tensor               # float64 [B, 3]: (ip, gd, iaf), the means over the row's own non-void terms
    counts: torch.Tensor             # int32 [B, 3]: the non-void terms of each mean
    status: torch.Tensor             # int32 [B]: bit i = term i has no non-void term (value 0, no gradient)
    g_real: Optional[torch.Tensor]   # float32, est_real's shape = dA / d est_real (exact zeros on void cells), or None
    g_imag: Optional[torch.Tensor]


def check_phase_settings(w_ip, w_gd, w_iaf, floor):
    """The settings of Engine.phase_loss / training.AuxLoss (pure host code): three finite weights >= 0 and a finite
    magnitude floor >= 0.  Returns four floats."""
    out = []
    for name, v in (("w_ip", w_ip), ("w_gd", w_gd), ("w_iaf", w_iaf), ("phase_floor", floor)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name}: expected a number, got {type(v).__name__}")
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name}: must be finite and >= 0, got {v}")
        out.append(float(v))
    return tuple(out)


def check_phase_loss_args(device, F, est_real, est_imag, clean_spec, w_ip=1.0, w_gd=1.0, w_iaf=1.0, floor=0.0):
    """Argument rules of Engine.phase_loss (pure host code); F is the Engine's.  Returns (B, T, w_ip, w_gd, w_iaf, floor)."""
    w_ip, w_gd, w_iaf, floor = check_phase_settings(w_ip, w_gd, w_iaf, floor)
    tensor_arg(est_real, "est_real", torch.float32, device, f"[B, T, {F}] or [B, 1, T, {F}]",
               lambda t: t.dim() in (3, 4) and (t.dim() == 3 or t.size(1) == 1) and t.size(0) >= 1 and t.size(-2) >= 1
               and t.size(-1) == F)
    shape = tuple(est_real.shape)
    B, T = int(shape[0]), int(shape[-2])
    tensor_arg(est_imag, "est_imag", torch.float32, device, f"{list(shape)}", lambda t: tuple(t.shape) == shape)
    tensor_arg(clean_spec, "clean_spec", torch.float32, device, f"[{B}, 2, {T}, {F}]", lambda t: tuple(t.shape) == (B, 2, T, F))
    if B > 65535:
        raise ValueError(f"est_real: at most 65535 rows, got {B}")
    if T > PHASE_MAX_T:
        raise ValueError(f"est_real: at most {PHASE_MAX_T} frames, got {T}")
    if F > PHASE_MAX_F:
        raise ValueError(f"est_real: at most {PHASE_MAX_F} bins, got {F}")
    return B, T, w_ip, w_gd, w_iaf, floor


def metric_frames(L: int, fs: int):
    """(WSS / segSNR frames, LLR frames) of an L-sample signal: the two counts of cmgan_amd.metrics."""
    win = int(np.round(30 * fs / 1000))
    hop = win // 4
    return int(L / hop - win / hop), int((L - win) / hop)


#: kernel families (names of _lib.MIX) that run ONE fp16 product in mfma_mode="f16mix".  The ablation
#: (tools/mix_ablation.py -> profiles/r06_mix_ablation.json, 32 x 2 s clips + three real recordings, error vs the F16X3
#: output): alone, every conformer family costs 1e-5 .. 7e-5 and the dense / sub-pixel convs 6e-4 .. 1.4e-3 - F16X1's whole
#: error is the convs.  All six conformer families together: 5.9e-5 (batch) / 1.14e-4 (recordings) for 18.1 vs 21.1 ms.
F16MIX_PRESET = ("ff1", "ff2", "qkv", "attn", "pw1", "dwpw2")


class Engine:
    """One handle = one device = one set of weights.  Not re-entrant: the workspace is shared by all calls,
    so use an Engine from ONE stream at a time (the stream current on its device when a method is called)."""

    def __init__(self, n_fft: int = 400, hop: int = 100, num_features: Optional[int] = None,
                 num_tscb: int = 4, max_pos_emb: int = 512, device: Optional[torch.device] = None,
                 mfma_mode: Optional[str] = None, mix_single=None):
        """mfma_mode: "f16x3" (default; fp32-accurate split products on the f16 matrix pipe), "f32" (bit-exact fp32
        MFMA), "f16x1" (REDUCED precision, opt-in: one fp16 product per contraction in the TSCNet body, 6e-4 .. 9e-4 of
        the peak vs the reference - inside the 1e-3 gate without margin, 200x the default mode's error) or "f16mix"
        (REDUCED precision, opt-in, WITH margin: only the kernel families in `mix_single` - names of _lib.MIX, default
        F16MIX_PRESET - run one product, the rest three; <= 2e-4 end to end) - see include/cmgan_hip.h."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("cmgan_amd needs a ROCm GPU: torch.cuda.is_available() is False")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise RuntimeError(f"cmgan_amd has no CPU path: device must be a GPU, got {self.device}")
        if self.device.index is None:
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        cfg = _lib.default_config()
        cfg.n_fft, cfg.hop = n_fft, hop
        cfg.num_features = num_features if num_features is not None else n_fft // 2 + 1
        cfg.num_tscb, cfg.max_pos_emb = num_tscb, max_pos_emb
        if mfma_mode is not None:
            modes = {"f32": _lib.MFMA_F32, "f16x3": _lib.MFMA_F16X3, "f16x1": _lib.MFMA_F16X1, "f16mix": _lib.MFMA_F16MIX}
            if mfma_mode not in modes:
                raise ValueError(f"mfma_mode must be one of {sorted(modes)}")
            cfg.mfma_mode = modes[mfma_mode]
        if mix_single is not None and cfg.mfma_mode != _lib.MFMA_F16MIX:
            raise ValueError("mix_single only applies to mfma_mode='f16mix'")
        if cfg.mfma_mode == _lib.MFMA_F16MIX:
            fams = F16MIX_PRESET if mix_single is None else tuple(mix_single)
            unknown = [f for f in fams if f not in _lib.MIX]
            if unknown:
                raise ValueError(f"unknown kernel families {unknown}: choose from {sorted(_lib.MIX)}")
            cfg.single_mask = sum(_lib.MIX[f] for f in set(fams))
            self.mix_single = tuple(sorted(set(fams)))
        self.mfma_mode = {_lib.MFMA_F32: "f32", _lib.MFMA_F16X3: "f16x3", _lib.MFMA_F16X1: "f16x1",
                          _lib.MFMA_F16MIX: "f16mix"}[cfg.mfma_mode]
        self.cfg = cfg
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.cmgan_create(ctypes.byref(self._h), ctypes.byref(cfg))
        if rc != 0:
            msg = self.lib.cmgan_last_error(None)
            raise _lib.CmganError(rc, msg.decode() if msg else "?")
        #: grow-only uint8 workspaces by name (_grow): "main", "branched" (enhance_graphed(branches > 1)), "conformer",
        #: "metrics", "mix", "scene", "rir", "rir_bands", "rir_dir", "rir_bands_dir", "level", "channel", "dynamics", "noise", "suppress", "aux_loss", "stoi_loss", "phase_loss" and ("resample", fs_in,
        #: fs_out), the rate pair's tap table
        self._wss: dict = {}
        self._graphs: dict = {}          # enhance_graphed: input shape -> (graph, in, out, token)
        self._row_graphs: dict = {}      # streaming.enhance_windows: row shape -> (graph, in, out, token)
        self._stream_slots: dict = {}    # streaming.StreamState(graph=True): (B, W, Ca, La, stats mode) -> state + step graphs
        self.weights_loaded = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.lib.cmgan_destroy(h)
            except Exception:
                pass
            self._h = ctypes.c_void_p()

    # ---- weights -------------------------------------------------------------------
    def load_blob(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        # cmgan_load_weights re-allocates the device weight buffers: every captured graph holds kernel arguments
        # pointing into the old ones, so they are dropped BEFORE the swap (a failed load keeps the old weights,
        # and the graphs are simply re-captured on next use)
        self._graphs.clear()
        self._row_graphs.clear()
        self._stream_slots.clear()
        with torch.cuda.device(self.device):
            native_call(self, "cmgan_load_weights", blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes)
        self.weights_loaded = True

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _in(self, t: torch.Tensor, name: str) -> torch.Tensor:
        return tensor_arg(t, name, torch.float32, self.device, contiguous=False).contiguous()

    def _call(self, name: str, *args) -> None:
        """One native call `name(handle, *args, stream)` (native_call) on the current stream of the engine's device, with
        that device current: the launch goes there whatever device the caller has current."""
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                return self._call(name, *args)
        native_call(self, name, *args, self._stream())

    # ---- workspace -----------------------------------------------------------------
    def _ws_token(self):
        """Identity of what a captured graph's kernel arguments point into: the workspace allocation and the
        weight buffers (cmgan_weights_generation).  A graph whose token differs is stale and is re-captured."""
        ws = self._wss.get("main")
        return (ws.data_ptr() if ws is not None else 0, ws.numel() if ws is not None else 0,
                int(self.lib.cmgan_weights_generation(self._h)))

    def _evict_main(self):
        # graphs captured on the old allocation are stale AND keep it (multi-GB) alive: evict them all
        self._graphs = {k: v for k, v in self._graphs.items() if k[1] != 1}
        self._row_graphs.clear()
        for slot in self._stream_slots.values():
            slot.graphs.clear()
            slot.stage_graphs.clear()

    def _evict_branched(self):
        self._graphs = {k: v for k, v in self._graphs.items() if k[1] == 1}

    #: what a slot's growth evicts first: the captured graphs whose kernel arguments point into its old allocation
    _EVICT = {"main": _evict_main, "branched": _evict_branched}

    def _grow(self, slot, need: int, bad: Optional[str] = None) -> torch.Tensor:
        """The grow-only workspace `slot`: its tensor when it holds `need` bytes, else a new one of that size (the old
        allocation is dropped first, so the peak is not old + new).  need == 0 with a message `bad`: ValueError(bad)."""
        if need == 0 and bad is not None:
            raise ValueError(bad)
        if slot not in self._wss or self._wss[slot].numel() < need:
            if slot in self._EVICT:
                self._EVICT[slot](self)
            self._wss.pop(slot, None)
            self._wss[slot] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._wss[slot]

    def _workspace(self, B: int, T: int) -> torch.Tensor:
        return self._grow("main", self.lib.cmgan_workspace_bytes(self._h, B, T), f"bad batch/frames ({B}, {T})")

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self.lib.cmgan_workspace_bytes(self._h, B, T))

    def _conf_workspace(self, N: int, L: int) -> torch.Tensor:
        return self._grow("conformer", self.lib.cmgan_conformer_workspace_bytes(self._h, N, L))

    @property
    def F(self) -> int:
        return self.cfg.num_features

    def num_frames(self, L: int) -> int:
        return L // self.cfg.hop + 1

    # ---- front / back end ----------------------------------------------------------
    @_on_device
    def rms_scale(self, wav: torch.Tensor) -> torch.Tensor:
        wav = self._in(wav, "wav")
        B, L = wav.shape
        out = torch.empty(B, dtype=torch.float32, device=wav.device)
        self._call("cmgan_rms_scale", wav, B, L, out)
        return out

    @_on_device
    def stft_compress(self, wav: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        wav = self._in(wav, "wav")
        B, L = wav.shape
        sp = self._in(scale, "scale") if scale is not None else None
        out = torch.empty(B, 2, self.num_frames(L), self.F, dtype=torch.float32, device=wav.device)
        self._call("cmgan_stft_compress", wav, sp, B, L, out)
        return out

    @_on_device
    def uncompress_istft(self, real: torch.Tensor, imag: torch.Tensor,
                         scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        real, imag = self._in(real, "real"), self._in(imag, "imag")
        B, T = self._est_shape(real, imag)
        ws = self._workspace(B, T)
        sp = self._in(scale, "scale") if scale is not None else None
        out = torch.empty(B, self.cfg.hop * (T - 1), dtype=torch.float32, device=real.device)
        self._call("cmgan_uncompress_istft", real, imag, sp, B, T, out, ws, ws.numel())
        return out

    @_on_device
    def power_compress(self, x: torch.Tensor) -> torch.Tensor:
        x = self._in(x, "x")
        if x.dim() != 4 or x.size(3) != 2:
            raise ValueError(f"expected [B,F,T,2], got {tuple(x.shape)}")
        B, F, T, _ = x.shape
        y = torch.empty(B, 2, F, T, dtype=torch.float32, device=x.device)
        self._call("cmgan_power_compress", x, B, F, T, y)
        return y

    @_on_device
    def power_uncompress(self, real: torch.Tensor, imag: torch.Tensor) -> torch.Tensor:
        real, imag = self._in(real, "real"), self._in(imag, "imag")
        B, one, F, T = real.shape
        y = torch.empty(B, 1, F, T, 2, dtype=torch.float32, device=real.device)
        self._call("cmgan_power_uncompress", real, imag, B, F, T, y)
        return y

    # ---- model ---------------------------------------------------------------------
    def _need_weights(self):
        if not self.weights_loaded:
            raise RuntimeError("no weights loaded: call load_state_dict() first")

    # ---- the model-layout tensors: spectrogram [B,2,T,F], features [B,T,F',64], estimate 2 x [B,1,T,F] ----
    def _spec_shape(self, x: torch.Tensor):
        if x.dim() != 4 or x.size(1) != 2 or x.size(3) != self.F:
            raise ValueError(f"expected [B,2,T,{self.F}], got {tuple(x.shape)}")
        return x.size(0), x.size(2)

    def _feat_shape(self, x: torch.Tensor):
        if x.dim() != 4 or x.size(2) != (self.F + 1) // 2 or x.size(3) != 64:
            raise ValueError(f"expected [B,T,{(self.F + 1) // 2},64], got {tuple(x.shape)}")
        return x.size(0), x.size(1)

    def _est_shape(self, real: torch.Tensor, imag: torch.Tensor):
        if real.dim() != 4 or real.size(3) != self.F or imag.shape != real.shape:
            raise ValueError(f"expected 2 x [B,1,T,{self.F}], got {tuple(real.shape)} / {tuple(imag.shape)}")
        return real.size(0), real.size(2)

    def _decoder_shape(self, x: torch.Tensor, spec: torch.Tensor):
        B, T = self._feat_shape(x)
        if self._spec_shape(spec) != (B, T):
            raise ValueError(f"x {tuple(x.shape)} and spec {tuple(spec.shape)} differ in batch or frames")
        return B, T

    def _est_pair(self, B: int, T: int):
        real = torch.empty(B, 1, T, self.F, dtype=torch.float32, device=self.device)
        return real, torch.empty_like(real)

    @_on_device
    def tscnet_forward(self, x: torch.Tensor, taps: bool = False):
        self._need_weights()
        x = self._in(x, "x")
        B, T = self._spec_shape(x)
        ws = self._workspace(B, T)
        real, imag = self._est_pair(B, T)
        if not taps:
            self._call("cmgan_tscnet_forward", x, B, T, real, imag, ws, ws.numel())
            return real, imag
        F, F2 = self.F, (self.F + 1) // 2
        st = {"encoder": torch.empty(B, 64, T, F2, dtype=torch.float32, device=x.device),
              "mask": torch.empty(B, 1, T, F, dtype=torch.float32, device=x.device),
              "complex": torch.empty(B, 2, T, F, dtype=torch.float32, device=x.device)}
        tp = Taps()
        tp.encoder_dev = st["encoder"].data_ptr()
        for k in range(self.cfg.num_tscb):
            st[f"tscb{k + 1}"] = torch.empty(B, 64, T, F2, dtype=torch.float32, device=x.device)
            tp.tscb_dev[k] = st[f"tscb{k + 1}"].data_ptr()
        tp.mask_dev, tp.complex_dev = st["mask"].data_ptr(), st["complex"].data_ptr()
        self._call("cmgan_tscnet_forward_taps", x, B, T, real, imag, tp, ws, ws.numel())
        return real, imag, st

    # ---- frozen-statistics / sliced forms (streaming with carried state; include/cmgan_hip.h, "Streaming") ----
    def stats_floats(self, B: int) -> int:
        return int(self.lib.cmgan_stats_floats(self._h, B))

    @_on_device
    def tscnet_forward_stats(self, x: torch.Tensor, frozen: Optional[torch.Tensor] = None, export: bool = True):
        """TSCNet.forward with every InstanceNorm on the `frozen` statistics blob (None = the tensor's own, i.e. the
        reference's arithmetic).  Returns (real, imag, blob of the statistics this call used or None)."""
        self._need_weights()
        x = self._in(x, "x")
        B, T = self._spec_shape(x)
        ws = self._workspace(B, T)
        real, imag = self._est_pair(B, T)
        out = torch.empty(self.stats_floats(B), dtype=torch.float32, device=x.device) if export else None
        self._call("cmgan_tscnet_forward_stats", x, B, T, real, imag, self._stats_arg(frozen, B), out, ws, ws.numel())
        return real, imag, out

    def _stats_arg(self, stats: Optional[torch.Tensor], B: int):
        if stats is None:
            return None
        stats = self._in(stats, "stats")
        if stats.numel() != self.stats_floats(B):
            raise ValueError(f"statistics blob has {stats.numel()} floats, a batch of {B} rows needs {self.stats_floats(B)}")
        return stats

    def _own_ws(self, ws: Optional[torch.Tensor], B: int, T: int) -> torch.Tensor:
        if ws is None:
            return self._workspace(B, T)
        need = self.workspace_bytes(B, T)
        return tensor_arg(ws, "ws", torch.uint8, self.device, f"at least workspace_bytes({B}, {T}) = {need} bytes",
                          lambda t: t.numel() >= need, error=ValueError)

    def _feat_out(self, out: Optional[torch.Tensor], B: int, T: int) -> torch.Tensor:
        """The [B,T,F',64] result of the stream encoders: a new tensor, or the caller's (the kernel writes it in place)."""
        want = (B, T, (self.F + 1) // 2, 64)
        if out is None:
            return torch.empty(want, dtype=torch.float32, device=self.device)
        return tensor_arg(out, "out", torch.float32, self.device, f"[B,T,F',64] = {want}", lambda t: tuple(t.shape) == want)

    @_on_device
    def stream_encoder(self, spec: torch.Tensor, stats: torch.Tensor, out: Optional[torch.Tensor] = None,
                       ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dense_encoder under frozen statistics: spec [B,2,T,F] -> x [B,T,F',64] (channels-last).  ws: a workspace of the
        caller's instead of the engine's (lets the call run on another stream beside a step's TSCBs)."""
        self._need_weights()
        spec = self._in(spec, "spec")
        B, T = self._spec_shape(spec)
        ws = self._own_ws(ws, B, T)
        out = self._feat_out(out, B, T)
        self._call("cmgan_stream_encoder", spec, B, T, self._stats_arg(stats, B), out, ws, ws.numel())
        return out

    @_on_device
    def stream_tscb(self, x: torch.Tensor) -> torch.Tensor:
        """TSCB_1..4 on x [B,T,F',64], IN PLACE (returns x)."""
        self._need_weights()
        if not x.is_contiguous():
            raise ValueError("stream_tscb works in place: x must be contiguous")
        x = self._in(x, "x")
        B, T = self._feat_shape(x)
        ws = self._workspace(B, T)
        self._call("cmgan_stream_tscb", x, B, T, ws, ws.numel())
        return x

    @_on_device
    def stream_decoder(self, x: torch.Tensor, spec: torch.Tensor, stats: torch.Tensor, ws: Optional[torch.Tensor] = None):
        """mask + complex decoder + recombination under frozen statistics: x [B,T,F',64], spec [B,2,T,F] ->
        (est_real, est_imag) [B,1,T,F].  ws: a workspace of the caller's (uint8, >= workspace_bytes(B, T)) instead of the
        engine's - what lets a decoder call run on another stream BESIDE the next step's encoder / TSCBs."""
        self._need_weights()
        x, spec = self._in(x, "x"), self._in(spec, "spec")
        B, T = self._decoder_shape(x, spec)
        ws = self._own_ws(ws, B, T)
        real, imag = self._est_pair(B, T)
        self._call("cmgan_stream_decoder", x, spec, B, T, self._stats_arg(stats, B), real, imag, ws, ws.numel())
        return real, imag

    # ---- running-statistics forms (include/cmgan_hip.h, "Streaming": running statistics) ----
    def stream_sums_doubles(self, B: int) -> int:
        return int(self.lib.cmgan_stream_sums_doubles(self._h, B))

    def _sums_arg(self, sums: torch.Tensor, B: int) -> torch.Tensor:
        n = self.stream_sums_doubles(B)
        return tensor_arg(sums, "sums", torch.float64, self.device, f"stream_sums_doubles({B}) = {n} elements",
                          lambda t: t.numel() == n, error=ValueError)

    def _stats_out_arg(self, stats_out: Optional[torch.Tensor], B: int) -> Optional[torch.Tensor]:
        if stats_out is None:
            return None
        n = self.stats_floats(B)
        return tensor_arg(stats_out, "stats_out", torch.float32, self.device, f"stats_floats({B}) = {n} elements",
                          lambda t: t.numel() == n, error=ValueError)

    @_on_device
    def stream_encoder_running(self, spec: torch.Tensor, hist: int, sums: torch.Tensor, out: Optional[torch.Tensor] = None,
                               ws: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """stream_encoder under RUNNING statistics: spec [B,2,T,F] whose first `hist` frames were counted by an earlier
        step -> x [B,T,F',64].  `sums` (float64, stream_sums_doubles(B)) is updated in place (norms 0..5);
        `stats_out` (float32, stats_floats(B)) receives the encoder's part of the statistics blob this call used."""
        self._need_weights()
        spec = self._in(spec, "spec")
        B, T = self._spec_shape(spec)
        ws = self._own_ws(ws, B, T)
        out = self._feat_out(out, B, T)
        self._call("cmgan_stream_encoder_running", spec, B, T, int(hist), self._sums_arg(sums, B),
                   self._stats_out_arg(stats_out, B), out, ws, ws.numel())
        return out

    @_on_device
    def stream_decoder_running(self, x: torch.Tensor, spec: torch.Tensor, hist: int, sums: torch.Tensor,
                               ws: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None):
        """stream_decoder under RUNNING statistics: x [B,T,F',64], spec [B,2,T,F], the first `hist` frames counted by an
        earlier step -> (est_real, est_imag) [B,1,T,F].  `sums` is updated in place (norms 6..15); `stats_out` receives
        the decoders' part of the statistics blob this call used."""
        self._need_weights()
        x, spec = self._in(x, "x"), self._in(spec, "spec")
        B, T = self._decoder_shape(x, spec)
        ws = self._own_ws(ws, B, T)
        real, imag = self._est_pair(B, T)
        self._call("cmgan_stream_decoder_running", x, spec, B, T, int(hist), self._sums_arg(sums, B),
                   self._stats_out_arg(stats_out, B), real, imag, ws, ws.numel())
        return real, imag

    @_on_device
    def conformer_forward(self, index: int, x: torch.Tensor, taps: bool = False, mask: Optional[torch.Tensor] = None):
        """mask: [N, L] bool (or any integer / float tensor, non-zero = keep) - ConformerBlock.forward(x, mask)."""
        self._need_weights()
        x = self._in(x, "x")
        N, L, C = x.shape
        if C != 64:
            raise ValueError("conformer dim must be 64")
        ws = self._conf_workspace(N, L)
        y = torch.empty_like(x)
        tp = torch.empty(4, N, L, 64, dtype=torch.float32, device=x.device) if taps else None
        if mask is None:
            self._call("cmgan_conformer_forward", index, x, N, L, y, tp, ws, ws.numel())
        else:
            if tuple(mask.shape) != (N, L):
                raise ValueError(f"mask must be [N, L] = [{N}, {L}], got {tuple(mask.shape)}")
            if mask.device != x.device:
                raise ValueError(f"mask is on {mask.device}, x on {x.device}")
            mk = (mask != 0).to(torch.uint8).contiguous()
            self._call("cmgan_conformer_forward_masked", index, x, N, L, mk, y, tp, ws, ws.numel())
        return (y, tp) if taps else y

    @_on_device
    def enhance(self, wav: torch.Tensor) -> torch.Tensor:
        """wav[B,L] -> enhanced[B,L]: the whole device pipeline in one ABI call."""
        self._need_weights()
        wav = self._in(wav, "wav")
        B, L = wav.shape
        ws = self._workspace(B, self.num_frames(L))
        out = torch.empty_like(wav)
        self._call("cmgan_enhance", wav, B, L, out, ws, ws.numel())
        return out

    # ---- hipGraph replay of the whole pipeline -------------------------------------------
    #: enhance_graphed's defaults (overridable per call and through CMGAN_BRANCHES / CMGAN_BRANCH_OFFSET): part-batch
    #: branches the captured graph holds, and the launches branch i issues before branch i + 1 starts.  Measured in one
    #: session at 32 x 2 s (profiles/r06_branch_sweep.txt): 1 branch 21.7 ms, 2 branches together 21.0 - 21.1 ms (-3 %),
    #: offsets of 12 / 24 / 60 launches 21.45 / 21.7 / 22.3 ms: what a second branch buys is the other branch's
    #: workgroups in every kernel's ramp-up and drain, not unlike kernels side by side.
    BRANCHES = 2
    BRANCH_OFFSET = 0
    MAX_BRANCHES = 8

    def _enhance_call(self, wav, out, B, L, branches: int, offset: int):
        if branches == 1:
            ws = self._workspace(B, self.num_frames(L))
            self._call("cmgan_enhance", wav, B, L, out, ws, ws.numel())
        else:
            ws = self._branched_workspace(B, self.num_frames(L), branches)
            with torch.cuda.device(self.device):           # (the one entry point whose stream is not its last argument)
                native_call(self, "cmgan_enhance_branched", wav, B, L, out, ws, ws.numel(), self._stream(), branches, offset)

    def _branched_workspace(self, B: int, T: int, branches: int) -> torch.Tensor:
        return self._grow("branched", self.lib.cmgan_workspace_bytes_branched(self._h, B, T, branches),
                          f"bad batch / frames / branches ({B}, {T}, {branches})")

    def _branch_args(self, B: int, branches: Optional[int], offset: Optional[int]):
        import os
        if branches is None:
            branches = int(os.environ.get("CMGAN_BRANCHES", self.BRANCHES))
        if offset is None:
            offset = int(os.environ.get("CMGAN_BRANCH_OFFSET", self.BRANCH_OFFSET))
        if not 1 <= branches <= self.MAX_BRANCHES:
            raise ValueError(f"branches must be 1 .. {self.MAX_BRANCHES}")
        if offset < 0:
            raise ValueError("branch offset must be >= 0")
        branches = min(branches, B)
        return branches, (offset if branches > 1 else 0)

    @_on_device
    def enhance_branched(self, wav: torch.Tensor, branches: int = 2, offset: int = 0) -> torch.Tensor:
        """enhance() as `branches` part-batch branches on as many streams (cmgan_enhance_branched); same result bit for bit."""
        self._need_weights()
        wav = self._in(wav, "wav")
        B, L = wav.shape
        out = torch.empty_like(wav)
        branches, offset = self._branch_args(B, branches, offset)
        self._enhance_call(wav, out, B, L, branches, offset)
        return out

    @_on_device
    def _capture(self, body, restore=(), stream=None):
        """body() captured into a hipGraph -> (graph, what body returned).  THE protocol of every captured graph here:
        warm-up outside capture on a side stream (allocator pools, workspace growth, first-launch set-up), with the
        device idle before and after; `restore` - the state a run of the body modifies - is put back after the warm-up
        and again after the capture.  `stream`: where the graph will be replayed (default: the current stream); it is
        captured there unless that is the device's default stream, which cannot capture - torch's own capture stream does
        it then.  The workspace may have grown in here: callers read _ws_token() AFTER this returns."""
        dev = self.device
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        torch.cuda.synchronize(dev)
        saved = [t.clone() for t in restore]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            body()
        stream.wait_stream(side)
        torch.cuda.synchronize(dev)
        for dst, src in zip(restore, saved):
            dst.copy_(src)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=None if stream == torch.cuda.default_stream(dev) else stream):
            outs = body()
        for dst, src in zip(restore, saved):                   # (capture does not execute, but keep the rule simple)
            dst.copy_(src)
        torch.cuda.synchronize(dev)
        return graph, outs

    @_on_device
    def enhance_graphed(self, wav: torch.Tensor, branches: Optional[int] = None, offset: Optional[int] = None) -> torch.Tensor:
        """Same result as enhance(), but the ~250 kernel launches of cmgan_enhance are captured once
        per input shape into a hipGraph (torch.cuda.CUDAGraph on the capture stream) and replayed:
        the C ABI never allocates or synchronises, so it is capturable as is.  The returned tensor is
        a static buffer that the next call with the same shape overwrites.
        branches > 1: the graph holds that many part-batch branches (cmgan_enhance_branched) as parallel paths the GPU
        overlaps; the result is the same bit for bit (rows are independent).  Defaults: BRANCHES / BRANCH_OFFSET."""
        self._need_weights()
        wav = self._in(wav, "wav")
        B, L = wav.shape
        branches, offset = self._branch_args(B, branches, offset)
        key = (tuple(wav.shape), branches, offset)
        # the workspace may grow (and evict every graph that points into it) first
        T = self.num_frames(L)
        ws = self._workspace(B, T) if branches == 1 else self._branched_workspace(B, T, branches)
        token = (ws.data_ptr(), ws.numel(), int(self.lib.cmgan_weights_generation(self._h)))
        ent = self._graphs.get(key)
        if ent is not None and ent[3] != token:                 # workspace or weights changed since capture
            ent = None
        if ent is None:
            g_in, g_out = torch.empty_like(wav), torch.empty_like(wav)
            g_in.copy_(wav)
            graph, _ = self._capture(lambda: self._enhance_call(g_in, g_out, B, L, branches, offset))
            ent = (graph, g_in, g_out, token)
            self._graphs[key] = ent
        graph, g_in, g_out, _ = ent
        g_in.copy_(wav)
        graph.replay()
        return g_out

    # ---- training / validation step pieces (src/train.py) ----------------------------------
    @_on_device
    def loss_terms(self, est_real=None, est_imag=None, clean_spec=None, est_audio=None, clean_audio=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """{loss_ri, loss_mag, time_loss, time_mse} of Trainer.calculate_generator_loss (train.py:124-151) as a
        float32[4] device tensor (deterministic two-pass reduction).  Spectral operands in the model layout:
        est_real/est_imag [B,1,T,F], clean_spec [B,2,T,F]; audio [B,L].  Either group may be omitted."""
        spec = [est_real, est_imag, clean_spec]
        audio = [est_audio, clean_audio]
        if any(t is None for t in spec) and not all(t is None for t in spec):
            raise ValueError("spectral terms need est_real, est_imag and clean_spec together")
        if any(t is None for t in audio) and not all(t is None for t in audio):
            raise ValueError("the time term needs est_audio and clean_audio together")
        B = T = L = 0
        if spec[0] is not None:
            spec = [self._in(t, n) for t, n in zip(spec, ("est_real", "est_imag", "clean_spec"))]
            B, T = self._est_shape(spec[0], spec[1])
            if self._spec_shape(spec[2]) != (B, T):
                raise ValueError(f"expected est [B,1,T,{self.F}] x2 and clean_spec [B,2,T,{self.F}]")
        if audio[0] is not None:
            audio = ea, ca = [self._in(audio[0], "est_audio"), self._in(audio[1], "clean_audio")]
            if ea.shape != ca.shape or ea.dim() != 2 or (B and ea.size(0) != B):
                raise ValueError("est_audio / clean_audio must both be [B, L]")
            B, L = ea.shape
        if out is None:
            out = torch.empty(4, dtype=torch.float32, device=self.device)
        self._call("cmgan_loss_terms", *spec, B, T, *audio, L, self._in(out, "out"))
        return out

    # ---- objective metrics ---------------------------------------------------------
    @_on_device
    def metrics(self, clean: torch.Tensor, enhanced: torch.Tensor, fs: int = 16000, pesq_mos=None,
                per_frame: bool = False):
        """Objective scores of B pairs on the GPU (cmgan_metrics; host twin: cmgan_amd.metrics.compute_metrics).

        clean, enhanced: float32 device tensors [B, L] (or [L]).  Unequal lengths are handled like the reference tool:
        both are trimmed to the shorter one and eps is added to every sample.  pesq_mos: a float or a [B] tensor (the
        composites need it; None gives NaN composites).  Returns DeviceScores of float64 [B] device tensors (pesq, csig,
        cbak, covl, ssnr, stoi, wss, llr, snr); with per_frame=True also FrameScores (wss [B, nf_wss], llr [B, nf_llr],
        segsnr [B, nf_wss]).  Needs no weights and does not synchronise."""
        clean, enhanced = self._in(clean, "clean"), self._in(enhanced, "enhanced")
        if clean.dim() == 1:
            clean = clean[None]
        if enhanced.dim() == 1:
            enhanced = enhanced[None]
        if clean.dim() != 2 or enhanced.dim() != 2 or clean.size(0) != enhanced.size(0):
            raise ValueError(f"expected two [B, L] tensors, got {tuple(clean.shape)} / {tuple(enhanced.shape)}")
        offset = 0.0
        if clean.size(1) != enhanced.size(1):                   # compute_metrics.py:41-44
            n = min(clean.size(1), enhanced.size(1))
            clean, enhanced = clean[:, :n].contiguous(), enhanced[:, :n].contiguous()
            offset = _EPS
        B, L = clean.shape
        need = int(self.lib.cmgan_metrics_workspace_bytes(self._h, B, L, fs))
        if need == 0:
            rc = self.lib.cmgan_metrics_table(fs, 0, None, 0)
            if rc < 0:
                raise _lib.CmganError(rc, f"unsupported sample rate {fs} (16000 or 8000)")
            raise ValueError(f"[{B}, {L}] at fs={fs} is too short to score (one 30-frame STOI window is needed)")
        ws = self._grow("metrics", need)
        pesq = None
        if pesq_mos is not None:
            if isinstance(pesq_mos, torch.Tensor):
                pesq = pesq_mos.to(device=self.device, dtype=torch.float64).reshape(-1).expand(B).contiguous()
            else:
                pesq = torch.full((B,), float(pesq_mos), dtype=torch.float64, device=self.device)
        scores = torch.empty(B, 9, dtype=torch.float64, device=self.device)
        nfw, nfl = metric_frames(L, fs)
        nf = max(nfw, nfl)
        frames = torch.empty(B, 3, nf, dtype=torch.float64, device=self.device) if per_frame else None
        self._call("cmgan_metrics", clean, enhanced, B, L, fs, pesq, offset, scores, frames, ws, ws.numel())
        out = DeviceScores(*scores.unbind(1))
        if not per_frame:
            return out
        return out, FrameScores(frames[:, 0, :nfw], frames[:, 1, :nfl], frames[:, 2, :nfw])

    # ---- sample-rate conversion ----------------------------------------------------
    def _resample_ws(self, fs_in: int, fs_out: int) -> torch.Tensor:
        ws = self._wss.get(("resample", fs_in, fs_out))
        if ws is None:
            need = int(self.lib.cmgan_resample_workspace_bytes(self._h, fs_in, fs_out))
            if need == 0:
                from .resample import geometry
                geometry(fs_in, fs_out)                       # raises CmganError with the library's message
            # one allocation per rate pair, kept: a captured graph's kernel arguments point into it
            ws = self._grow(("resample", fs_in, fs_out), need)
        return ws

    @_on_device
    def resample_chunk(self, buf: torch.Tensor, pos_in: int, fs_in: int, fs_out: int, n0: int, n_out: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Outputs [n0, n0 + n_out) of the resampled signal whose samples [pos_in, pos_in + n) `buf` [B, n] holds (samples
        it does not hold count as zero) -> [B, n_out].  The chunk form of resample(): same kernel, same bits."""
        buf = self._in(buf, "buf")
        if buf.dim() != 2:
            raise ValueError(f"expected [B, n], got {tuple(buf.shape)}")
        fs_in, fs_out = int(fs_in), int(fs_out)
        B, n_buf = buf.shape
        ws = self._resample_ws(fs_in, fs_out)
        if out is None:
            out = torch.empty(B, n_out, dtype=torch.float32, device=self.device)
        else:
            tensor_arg(out, "out", torch.float32, self.device, f"[{B}, {n_out}]", lambda t: tuple(t.shape) == (B, n_out),
                       error=ValueError)
        if B == 0 or n_out == 0:
            return out
        if n_buf == 0:                                        # no sample at all: every output is a sum of zeros
            return out.zero_()
        self._call("cmgan_resample", buf, B, n_buf, n_buf, int(pos_in), fs_in, fs_out, int(n0), int(n_out), out, n_out, ws,
                   ws.numel())
        return out

    def resample(self, wav: torch.Tensor, fs_in: int, fs_out: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wav [B, L] (or [L]) at fs_in -> [B, ceil(L up / down)] at fs_out on the GPU (cmgan_resample): the arithmetic
        of scipy.signal.resample_poly(wav, up, down) in float64, rounded to float32 once.  Supported: rate pairs whose
        reduced max(up, down) <= 640.  Needs no weights, does not synchronise and is graph-capturable after one call."""
        from .resample import out_len
        squeeze = isinstance(wav, torch.Tensor) and wav.dim() == 1
        if squeeze:
            wav = wav[None]
        y = self.resample_chunk(wav, 0, fs_in, fs_out, 0, out_len(fs_in, fs_out, wav.size(-1)), out=out)
        return y[0] if squeeze else y

    # ---- dynamic mixing ------------------------------------------------------------
    @_on_device
    def mix(self, clean: torch.Tensor, noise_bank: torch.Tensor, noise_start: torch.Tensor, noise_len: torch.Tensor,
            noise_off: torch.Tensor, snr_db: torch.Tensor, rir_bank: Optional[torch.Tensor] = None,
            rir_index: Optional[torch.Tensor] = None, rir_len: Optional[torch.Tensor] = None, peak: float = 0.99,
            early: int = -1):
        """Noisy (and reverberant) training pairs from clean speech on the GPU (cmgan_mix, include/cmgan_hip.h).

        clean float32 [B, L]; noise_bank flat float32 with int64 [B] noise_start / noise_len / noise_off (row b loops
        over bank[start : start + len] from offset off); snr_db float32 [B]; optionally rir_bank float32 [R, Kmax]
        (zero-padded rows) with int32 [B] rir_index / rir_len.  All on this Engine's device; the per-row tensors are read
        by the kernels only.  `early`: samples of early reflections kept in the target, -1 for the dry clip.
        Returns (noisy [B, L], target [B, L], MixInfo of float64 [B]).  Float64 arithmetic, one rounding to float32;
        bit-reproducible, row-independent, no synchronisation, graph-capturable after one call at the shape."""
        B, L, R, Kmax = check_mix_args(self.device, clean, noise_bank, noise_start, noise_len, noise_off, snr_db, rir_bank,
                                       rir_index, rir_len, peak, early)
        ws = self._grow("mix", int(self.lib.cmgan_mix_workspace_bytes(self._h, B, L, max(Kmax, 1))),
                        f"[{B}, {L}] with {Kmax} taps is outside what cmgan_mix supports")
        noisy = torch.empty(B, L, dtype=torch.float32, device=self.device)
        target = torch.empty(B, L, dtype=torch.float32, device=self.device)
        info = torch.empty(4, B, dtype=torch.float64, device=self.device)
        self._call("cmgan_mix", clean, B, L, L, noise_bank, noise_bank.numel(), noise_start, noise_len, noise_off, rir_bank, R,
                   Kmax, rir_index, rir_len, snr_db, float(peak), int(early), noisy, target, L, info[0], info[1], info[2],
                   info[3], ws, ws.numel())
        return noisy, target, MixInfo(info[0], info[1], info[2], info[3])

    # ---- scenes: located sources ----------------------------------------------------
    @_on_device
    def scene(self, clean: torch.Tensor, noise_bank: Optional[torch.Tensor] = None, noise_start: Optional[torch.Tensor] = None,
              noise_len: Optional[torch.Tensor] = None, noise_off: Optional[torch.Tensor] = None,
              snr_db: Optional[torch.Tensor] = None, n_src: Optional[torch.Tensor] = None,
              src_bank: Optional[torch.Tensor] = None, src_start: Optional[torch.Tensor] = None,
              src_len: Optional[torch.Tensor] = None, src_off: Optional[torch.Tensor] = None,
              src_snr_db: Optional[torch.Tensor] = None, rir_bank: Optional[torch.Tensor] = None,
              rir_index: Optional[torch.Tensor] = None, rir_len: Optional[torch.Tensor] = None,
              src_rir_index: Optional[torch.Tensor] = None, src_rir_len: Optional[torch.Tensor] = None, peak: float = 0.99,
              early: int = -1):
        """Engine.mix with point noise sources and interfering talkers inside the room (cmgan_scene, include/cmgan_hip.h).

        clean, the dry noise (noise_bank .. snr_db; all None: no dry noise), the talker's rir_bank / rir_index / rir_len,
        peak and early are Engine.mix's.  The located sources: n_src int32 [B], how many of the S <= 4 table columns a row
        uses (clamped to [0, S]; None: no sources, and no other src_ argument); src_bank flat float32 - the noise bank
        again, or a bank of speech for interfering talkers; src_start / src_len / src_off int64 [B, S], the looping
        segment of each source; src_snr_db float32 [B, S], the speech-to-source ratio; with a rir_bank src_rir_index /
        src_rir_len int32 [B, S], rows of the same bank (without one the sources are dry).  Source j of row b is its
        segment, looping both ways, convolved with its response WITHOUT delay removal and scaled to its SNR.  The columns
        beyond a row's n_src are never read.  All on this Engine's device; the tables are read by the kernels only.
        Returns (noisy [B, L], target [B, L], SceneInfo).  Float64 arithmetic, one rounding to float32; bit-reproducible,
        row-independent, no synchronisation, graph-capturable after one call at the shape; with n_src=None and a dry
        noise the outputs are Engine.mix's, bit for bit."""
        B, L, R, Kmax, S = check_scene_args(self.device, clean, noise_bank, noise_start, noise_len, noise_off, snr_db, n_src,
                                            src_bank, src_start, src_len, src_off, src_snr_db, rir_bank, rir_index, rir_len,
                                            src_rir_index, src_rir_len, peak, early)
        ws = self._grow("scene", int(self.lib.cmgan_scene_workspace_bytes(self._h, B, L, max(Kmax, 1), S)),
                        f"[{B}, {L}] with {Kmax} taps and {S} sources is outside what cmgan_scene supports")
        noisy = torch.empty(B, L, dtype=torch.float32, device=self.device)
        target = torch.empty(B, L, dtype=torch.float32, device=self.device)
        gp = torch.empty(2, B, 1 + S, dtype=torch.float64, device=self.device)
        info = torch.empty(2, B, dtype=torch.float64, device=self.device)
        self._call("cmgan_scene", clean, B, L, L, noise_bank, noise_bank.numel() if noise_bank is not None else 0,
                   noise_start, noise_len, noise_off, snr_db, src_bank, src_bank.numel() if src_bank is not None else 0, S,
                   n_src, src_start, src_len, src_off, src_snr_db, rir_bank, R, Kmax, rir_index, rir_len, src_rir_index,
                   src_rir_len, float(peak), int(early), noisy, target, L, gp[0], gp[1], info[0], info[1], ws, ws.numel())
        return noisy, target, SceneInfo(gp[0], info[1], info[0], gp[1])

    # ---- paths: a talker and sources that move ---------------------------------------
    @_on_device
    def scene_path(self, clean: torch.Tensor, hop: int, n_path: torch.Tensor, rir_bank: torch.Tensor, rir_index: torch.Tensor,
                   rir_len: torch.Tensor, noise_bank: Optional[torch.Tensor] = None, noise_start: Optional[torch.Tensor] = None,
                   noise_len: Optional[torch.Tensor] = None, noise_off: Optional[torch.Tensor] = None,
                   snr_db: Optional[torch.Tensor] = None, n_src: Optional[torch.Tensor] = None,
                   src_bank: Optional[torch.Tensor] = None, src_start: Optional[torch.Tensor] = None,
                   src_len: Optional[torch.Tensor] = None, src_off: Optional[torch.Tensor] = None,
                   src_snr_db: Optional[torch.Tensor] = None, src_n_path: Optional[torch.Tensor] = None,
                   src_rir_index: Optional[torch.Tensor] = None, src_rir_len: Optional[torch.Tensor] = None,
                   peak: float = 0.99, early: int = -1):
        """Engine.scene for a talker and sources that MOVE: a path of responses each (cmgan_scene_path, include/cmgan_hip.h).

        rir_index / rir_len are int32 [B, P], 1 <= P <= 64: waypoint p of row b is that row of rir_bank and sits at input
        sample p * hop; n_path int32 [B] is how many of the P columns the row uses (clamped to [1, P]; 1: it stands
        still).  The responses of neighbouring waypoints are cross-faded linearly by emission time, each with its OWN
        direct-path delay removed, so the speech stays aligned with the dry clip; Doppler is not modelled.  With n_src the
        sources take src_n_path int32 [B, S] and src_rir_index / src_rir_len int32 [B, S, P] the same way (their delay
        stays).  Everything else is Engine.scene's, and so is what comes back: (noisy [B, L], target [B, L], SceneInfo).
        A row whose n_path and src_n_path are 1 has the bits of Engine.scene with column 0 of the tables.  Float64
        arithmetic, one rounding to float32; bit-reproducible, row-independent, no synchronisation, graph-capturable
        after one call at the shape; the columns beyond a row's own count are never read."""
        B, L, R, Kmax, S, P = check_scene_path_args(self.device, clean, hop, n_path, rir_bank, rir_index, rir_len, noise_bank,
                                                    noise_start, noise_len, noise_off, snr_db, n_src, src_bank, src_start,
                                                    src_len, src_off, src_snr_db, src_n_path, src_rir_index, src_rir_len, peak,
                                                    early)
        ws = self._grow("scene_path", int(self.lib.cmgan_scene_path_workspace_bytes(self._h, B, L, Kmax, S, P)),
                        f"[{B}, {L}] with {Kmax} taps, {S} sources and {P} waypoints is outside what cmgan_scene_path supports")
        noisy = torch.empty(B, L, dtype=torch.float32, device=self.device)
        target = torch.empty(B, L, dtype=torch.float32, device=self.device)
        gp = torch.empty(2, B, 1 + S, dtype=torch.float64, device=self.device)
        info = torch.empty(2, B, dtype=torch.float64, device=self.device)
        self._call("cmgan_scene_path", clean, B, L, L, noise_bank, noise_bank.numel() if noise_bank is not None else 0,
                   noise_start, noise_len, noise_off, snr_db, src_bank, src_bank.numel() if src_bank is not None else 0, S,
                   n_src, src_start, src_len, src_off, src_snr_db, rir_bank, R, Kmax, P, int(hop), n_path, rir_index, rir_len,
                   src_n_path, src_rir_index, src_rir_len, float(peak), int(early), noisy, target, L, gp[0], gp[1], info[0],
                   info[1], ws, ws.numel())
        return noisy, target, SceneInfo(gp[0], info[1], info[0], gp[1])

    # ---- room impulse responses ----------------------------------------------------
    def _rir_out(self, R, K):
        """The (rir float32 [R, K], length int32 [R]) pair that Engine.rir and Engine.rir_bands return."""
        return (torch.empty(R, K, dtype=torch.float32, device=self.device),
                torch.empty(R, dtype=torch.int32, device=self.device))

    @_on_device
    def rir(self, rooms: torch.Tensor, n_taps: torch.Tensor, K: int, n_images, fs: int = 16000, c: float = 343.0,
            tw: int = 40, out=None, orient: Optional[torch.Tensor] = None, pattern: Optional[torch.Tensor] = None):
        """Room impulse responses of shoe-box rooms by the image-source method (cmgan_rir, include/cmgan_hip.h).

        rooms float64 [R, 15] (size Lx Ly Lz in metres, source, receiver, reflection coefficients bx0 bx1 by0 by1 bz0
        bz1) and n_taps int32 [R], both on this Engine's device and read by the kernels only; K taps per row of the
        result; n_images = (Nx, Ny, Nz), the image index range per axis; fs in Hz, c the speed of sound in m/s, tw the
        half-width of the windowed-sinc fractional-delay filter in samples.  `out` = (float32 [R, K], int32 [R]) is
        written in place.  Returns (rir float32 [R, K], length int32 [R]): exactly the `rir_bank` / `rir_len` source of
        Engine.mix.  Row r holds clamp(n_taps[r], 1, K) taps and zeros after them; an invalid row (a non-finite entry, a
        size <= 0, a coefficient outside [0, 1]) is zeros with length 1.  Float64 arithmetic, one rounding to float32;
        bit-reproducible, row-independent, no synchronisation, graph-capturable after one call at the shape.

        `orient` float64 [R, 6] and `pattern` float64 [R, 1, 2] (or [R, 2]), both or neither, make the two ends
        directional (cmgan_rir_dir): the source's facing vector then the receiver's, of any length, and the first-order
        coefficients alpha_s, alpha_m in [0, 1] (1 omni, 0.5 cardioid, 0 figure-of-eight).  A row whose alphas are both 1
        has the bits of the call without the tables; a non-finite entry, an alpha outside [0, 1], a component beyond
        1e100 or a zero vector at an end with alpha < 1 makes the row invalid."""
        R, K, N = check_rir_args(self.device, rooms, n_taps, K, n_images, fs, c, tw, out)
        orient, pattern = check_rir_dir_args(self.device, R, 1, orient, pattern)
        if orient is None:
            ws = self._grow("rir", int(self.lib.cmgan_rir_workspace_bytes(self._h, R, K, int(tw))),
                            f"[{R}, {K}] with tw = {tw} is outside what cmgan_rir supports")
            rir, length = out if out is not None else self._rir_out(R, K)
            self._call("cmgan_rir", rooms, n_taps, R, K, int(fs), float(c), int(tw), N[0], N[1], N[2], rir, K, length, ws,
                       ws.numel())
            return rir, length
        ws = self._grow("rir_dir", int(self.lib.cmgan_rir_dir_workspace_bytes(self._h, R, K, int(tw))),
                        f"[{R}, {K}] with tw = {tw} is outside what cmgan_rir_dir supports")
        rir, length = out if out is not None else self._rir_out(R, K)
        self._call("cmgan_rir_dir", rooms, orient, pattern, n_taps, R, K, int(fs), float(c), int(tw), N[0], N[1], N[2], rir, K,
                   length, ws, ws.numel())
        return rir, length

    @_on_device
    def rir_bands(self, rooms: torch.Tensor, bands: torch.Tensor, n_taps: torch.Tensor, K: int, filters: torch.Tensor,
                  n_images, fs: int = 16000, c: float = 343.0, tw: int = 40, out=None, orient: Optional[torch.Tensor] = None,
                  pattern: Optional[torch.Tensor] = None):
        """Room impulse responses with frequency-dependent walls and air absorption (cmgan_rir_bands, include/cmgan_hip.h):
        Engine.rir simulated in NB frequency bands at once - one image list, one accumulator per band - and joined by a
        filterbank.

        rooms float64 [R, 15] as for Engine.rir (its six coefficients are not read); bands float64 [R, NB, 7], per band
        the six reflection coefficients and the air attenuation m >= 0 in nepers per metre; n_taps int32 [R]; filters
        float64 [NB, NF], NF odd, one FIR per band (`mixing.octave_filterbank`), whose delay (NF - 1) / 2 is taken out;
        all on this Engine's device and read by the kernels only.  n_images must cover K + (NF - 1) / 2 taps.  `out` =
        (float32 [R, K], int32 [R]) is written in place.  Returns (rir float32 [R, K], length int32 [R]), as Engine.rir
        does.  An invalid row (a non-finite entry in columns 0 - 8 or in its band table, a size <= 0, a coefficient
        outside [0, 1], a negative m) is zeros with length 1.  Float64 arithmetic, one rounding to float32;
        bit-reproducible, row-independent, no synchronisation, graph-capturable after one call at the shape.

        `orient` float64 [R, 6] and `pattern` float64 [R, NB, 2], both or neither, make the two ends directional
        (cmgan_rir_bands_dir) as for Engine.rir, with one (alpha_s, alpha_m) pair per band."""
        R, K, N, NB, NF = check_rir_bands_args(self.device, rooms, bands, n_taps, K, filters, n_images, fs, c, tw, out)
        orient, pattern = check_rir_dir_args(self.device, R, NB, orient, pattern)
        name = "cmgan_rir_bands" if orient is None else "cmgan_rir_bands_dir"
        ws = self._grow(name[6:], int(getattr(self.lib, name + "_workspace_bytes")(self._h, R, K, int(tw), NB, NF)),
                        f"[{R}, {K}] with tw = {tw}, {NB} bands and {NF} filter taps is outside what {name} supports")
        rir, length = out if out is not None else self._rir_out(R, K)
        tables = (rooms, bands) if orient is None else (rooms, bands, orient, pattern)
        self._call(name, *tables, n_taps, R, K, NB, filters, NF, int(fs), float(c), int(tw), N[0], N[1], N[2], rir, K, length,
                   ws, ws.numel())
        return rir, length

    @_on_device
    def rir_stats(self, rir: torch.Tensor, length: Optional[torch.Tensor] = None, filters: Optional[torch.Tensor] = None,
                  fs: int = 16000, direct_ms: float = 2.5, edc: bool = False):
        """What every response of a bank measures as (cmgan_rir_stats, include/cmgan_hip.h): the Schroeder decay curve and
        the room-acoustic parameters of ISO 3382-1 as its published description gives them, on the GPU.

        rir float32 [R, K] (rows contiguous, any row stride >= K, K <= 65536) and length int32 [R] (None: every row has K
        samples; clamped to [1, K]; samples from a row's length on are never read), as Engine.rir returns them; filters
        float64 [NB, NF], NF odd, the filterbank of Engine.rir_bands (`mixing.octave_filterbank`) or None for the
        broad-band analysis alone; all on this Engine's device and read by the kernels only.  direct_ms is the half-width
        of the window around the strongest sample that counts as the direct sound.  Returns RirStats of float64 [R, NB +
        1] tensors, column 0 broad-band and column 1 + b band b: energy, direct (the index of the strongest sample),
        drr_db, c50_db, c80_db, d50, ts, edt, t20, t30, and the int32 status.  A time that cannot be fitted - the curve
        does not fall far enough within the row (no noise-floor compensation is done) - is NaN with its status bit set;
        a row with a non-finite sample is NaN throughout, a silent one NaN but for energy = 0.  edc=True returns
        (RirStats, the decay curve float64 [R, NB + 1, K], zeros from a row's length on).  Float64 arithmetic;
        bit-reproducible, row-independent, no synchronisation, graph-capturable after one call at the shape."""
        R, K, NB, NF = check_rir_stats_args(self.device, rir, length, filters, fs, direct_ms)
        ws = self._grow("rir_stats", int(self.lib.cmgan_rir_stats_workspace_bytes(self._h, R, K, NB, NF)),
                        f"[{R}, {K}] with {NB} bands and {NF} filter taps is outside what cmgan_rir_stats supports")
        stats = torch.empty(R, NB + 1, RIR_STATS_COLUMNS, dtype=torch.float64, device=self.device)
        status = torch.empty(R, NB + 1, dtype=torch.int32, device=self.device)
        curve = torch.empty(R, NB + 1, K, dtype=torch.float64, device=self.device) if edc else None
        self._call("cmgan_rir_stats", rir, R, K, rir.stride(0) if R > 1 else K, length, filters, NB, NF, int(fs),
                   float(direct_ms), stats, status, curve, ws, ws.numel())
        out = RirStats(*stats.unbind(dim=2), status)
        return (out, curve) if edc else out

    @_on_device
    def rir_tail(self, rir: torch.Tensor, length: torch.Tensor, n_taps: torch.Tensor, decay: torch.Tensor, seed: torch.Tensor,
                 filters: Optional[torch.Tensor] = None, fs: int = 16000, window_ms: float = 30.0):
        """The diffuse reverberant tail behind the early part of every response of a bank (cmgan_rir_tail,
        include/cmgan_hip.h): from its junction on, a row is extended IN PLACE by decaying noise that follows the given
        60 dB decay time band by band, its level fitted to the `window_ms` in front of the junction.

        rir float32 [R, K] (rows contiguous, any row stride >= K) and length int32 [R], as Engine.rir / Engine.rir_bands
        return them for a SHORT n_taps: length is the junction (clamped to [1, K]), below which the row is never written;
        n_taps int32 [R], the wanted total length; decay float64 [R, max(NB, 1)] seconds; seed int64 [R], one noise key per
        row; filters float64 [NB, NF], NF odd, the filterbank of Engine.rir_bands, or None for one broad band; all on this
        Engine's device and read by the kernels only.  Returns (rir, length, RirTail(gain, status)): the bank and its
        lengths updated in place, the fitted level per band and the int32 status.  A row with nothing to add, with a
        window that does not fit in front of its junction ((NF - 1) / 2 more with filters), with a decay time that is not
        finite and > 0 or with a non-finite sample in the fit's reach keeps its taps and length and gets gain 0 and the
        RIR_TAIL_* bits of the reasons.  Float64 arithmetic, one rounding to float32; bit-reproducible, row-independent,
        no synchronisation, graph-capturable after one call at the shape."""
        R, K, NB, NF, W = check_rir_tail_args(self.device, rir, length, n_taps, decay, seed, filters, fs, window_ms)
        ws = self._grow("rir_tail", int(self.lib.cmgan_rir_tail_workspace_bytes(self._h, R, K, NB, NF)),
                        f"[{R}, {K}] with {NB} bands and {NF} filter taps is outside what cmgan_rir_tail supports")
        gain = torch.empty(R, max(NB, 1), dtype=torch.float64, device=self.device)
        status = torch.empty(R, dtype=torch.int32, device=self.device)
        self._call("cmgan_rir_tail", rir, R, K, rir.stride(0) if R > 1 else K, length, n_taps, decay, seed, filters, NB, NF, W,
                   int(fs), status, gain, ws, ws.numel())
        return rir, length, RirTail(gain, status)

    # ---- active speech level -------------------------------------------------------
    @_on_device
    def speech_level(self, wav: torch.Tensor, lengths: Optional[torch.Tensor] = None, fs: int = 16000, counts: bool = False):
        """The active speech level of every row of a batch on the GPU (cmgan_speech_level, include/cmgan_hip.h): the level
        meter of ITU-T P.56, method B, as its published description gives it - not compared with ITU's own program.

        wav float32 [B, L] (rows contiguous, any row stride >= L); lengths int32 [B] on this Engine's device, read by the
        kernels only (None: every row has L samples; samples from a row's length on are never read); fs in 8000 .. 192000.
        Returns SpeechLevel(ms, active_ms, activity) of float64 [B]: the mean square, the mean square over the active time
        (200 ms hangover included) and their ratio.  All three are 0 where no speech is detected and NaN where the row
        holds a non-finite sample.  counts=True adds an int64 [B, 16] tensor: the active samples per threshold
        2^-15 .. 2^-1 and the row's length.  Float64 arithmetic; bit-reproducible, row-independent, no synchronisation,
        graph-capturable after one call at the shape."""
        B, L = check_level_args(self.device, wav, lengths, fs)
        ws = self._grow("level", int(self.lib.cmgan_speech_level_workspace_bytes(B, L)),
                        f"[{B}, {L}] is outside what cmgan_speech_level supports")
        level = torch.empty(B, 3, dtype=torch.float64, device=self.device)
        cnt = torch.empty(B, 16, dtype=torch.int64, device=self.device) if counts else None
        self._call("cmgan_speech_level", wav, B, L, wav.stride(0) if B > 1 else L, lengths, int(fs), level, cnt, ws,
                   ws.numel())
        out = SpeechLevel(level[:, 0], level[:, 1], level[:, 2])
        return (out, cnt) if counts else out

    # ---- recording channel ---------------------------------------------------------
    @_on_device
    def channel(self, wav: torch.Tensor, sos: torch.Tensor, n_sections: Optional[torch.Tensor] = None,
                clip: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, status: bool = False):
        """A recording channel per row on the GPU (cmgan_channel, include/cmgan_hip.h): a cascade of up to 8 biquads - an
        equaliser or microphone response, a band limit - and a clipping level.

        wav float32 [B, L] (rows contiguous, any row stride >= L); sos float64 [B, S, 6] in scipy's layout (b0 b1 b2 a0 a1
        a2 with a0 = 1; cmgan_amd.mixing has the designs); n_sections int32 [B]: how many of its S sections a row uses
        (None: all; 0 copies the row); clip float64 [B]: |y| is limited to it (None or +inf: no clipping); lengths int32 [B]
        (None: every row has L samples; samples from a row's length on are never read, and come out as zeros).  All on
        this Engine's device and read by the kernels only.  `out` float32 [B, L] is written in place of a new tensor;
        out=wav runs in place.  Returns the float32 [B, L] result, the arithmetic of scipy.signal.sosfilt in float64 with
        one rounding to float32; status=True adds an int32 [B] tensor, 1 for the rows that are invalid (a non-finite
        coefficient, a0 != 1, an unstable section, n_sections outside [0, S], clip NaN or <= 0) and come out as zeros.
        Bit-reproducible, row-independent (also of S beyond a row's own sections), no synchronisation, graph-capturable
        after one call at the shape."""
        B, L, S = check_channel_args(self.device, wav, sos, n_sections, clip, lengths, out)
        ws = self._grow("channel", int(self.lib.cmgan_channel_workspace_bytes(B, L, S)),
                        f"[{B}, {L}] with {S} sections is outside what cmgan_channel supports")
        if out is None:
            out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        st = torch.empty(B, dtype=torch.int32, device=self.device) if status else None
        self._call("cmgan_channel", wav, B, L, wav.stride(0) if B > 1 else L, lengths, sos, n_sections, S, clip, out,
                   out.stride(0) if B > 1 else L, st, ws, ws.numel())
        return (out, st) if status else out

    # ---- dynamics: compressor, limiter, automatic gain control ----------------------
    @_on_device
    def dynamics(self, wav: torch.Tensor, dyn: torch.Tensor, key: Optional[torch.Tensor] = None,
                 lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, info: bool = False):
        """A gain control per row on the GPU (cmgan_dynamics, include/cmgan_hip.h): the feed-forward compressor in the log
        domain with separate attack and release times - a compressor, a limiter (slope 1) or an AGC by its parameters.

        wav float32 [B, L] (rows contiguous, any row stride >= L); dyn float64 [B, 6] = (thr_db, slope, knee_db, a_att,
        a_rel, makeup_db) per row (cmgan_amd.mixing.dynamics_params makes it from ratios and milliseconds); key float32
        [B, L]: the signal whose level drives the gain (None: wav itself); lengths int32 [B] (None: every row has L samples;
        samples from a row's length on are never read, and come out as zeros).  All on this Engine's device and read by
        the kernels only.  `out` float32 [B, L] is written in place of a new tensor; out=wav runs in place, out=key is
        allowed, any other overlap of out with wav or key is a ValueError.  Returns the float32 [B, L] result: float64
        arithmetic with one rounding to float32.  info=True adds (status, peak_reduction_db): int32 [B], 1 for the rows that
        are invalid (a non-finite entry, slope outside [0, 1], knee < 0, a coefficient outside [0, 1), a length outside
        [0, L]) and come out as zeros, and float64 [B], the largest gain reduction of the row in dB.  A row with slope 0
        and makeup 0 is copied bit for bit.  Bit-reproducible, row-independent, no synchronisation, graph-capturable after
        one call at the shape."""
        B, L = check_dynamics_args(self.device, wav, dyn, key, lengths, out)
        ws = self._grow("dynamics", int(self.lib.cmgan_dynamics_workspace_bytes(B, L)),
                        f"[{B}, {L}] is outside what cmgan_dynamics supports")
        if out is None:
            out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        st = torch.empty(B, dtype=torch.int32, device=self.device) if info else None
        pk = torch.empty(B, dtype=torch.float64, device=self.device) if info else None
        self._call("cmgan_dynamics", wav, B, L, wav.stride(0) if B > 1 else L, key,
                   0 if key is None else (key.stride(0) if B > 1 else L), lengths, dyn, out, out.stride(0) if B > 1 else L,
                   st, pk, ws, ws.numel())
        return (out, st, pk) if info else out

    # ---- synthetic noise -------------------------------------------------------------
    @_on_device
    def noise(self, seed: torch.Tensor, fir: torch.Tensor, n: int, lengths: Optional[torch.Tensor] = None,
              start: Optional[torch.Tensor] = None, env: Optional[torch.Tensor] = None, env_hop: Optional[int] = None,
              tones: Optional[torch.Tensor] = None, n_tones: Optional[torch.Tensor] = None,
              impulse: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, info: bool = False):
        """Synthetic noise on the GPU (cmgan_noise, include/cmgan_hip.h): per row a unit-variance Philox noise - with clicks -
        coloured by the row's own FIR filter, under a piecewise-linear envelope, plus a sum of tones (a hum).

        seed int64 [N], one noise key per row; fir float64 [N, NF], 1 <= NF <= 1023 (cmgan_amd.mixing.noise_fir designs it
        from a magnitude); n: the samples per row; lengths int32 [N] (None: n; columns from a row's length on come out as
        zeros); start int64 [N]: the absolute index of a row's first sample (None: 0); env float64 [N, P], P <= 4096, the
        gain at points `env_hop` samples apart, interpolated linearly, the last point holding (None: 1); tones float64
        [N, M, 3] = (cycles per sample in [0, 0.5], amplitude, phase in cycles), M <= 8, of which row r uses the first
        n_tones[r] (int32 [N]; None: all M); impulse float64 [N, 2] = (thr, amplitude): an index carries a click, uniform
        in +-amplitude, with probability thr / 2^32, thr a whole number in [0, 2^32) (None: no clicks).  All on this
        Engine's device and read by the kernels only.  `out` float32 [N, n] (rows contiguous, any row stride >= n) is
        written in place of a new tensor.  Returns the float32 [N, n] result: float64 arithmetic with one rounding to
        float32; info=True adds the int32 [N] status, 1 for the rows that are invalid (a non-finite table entry, a length
        outside [0, n], n_tones outside [0, M], a frequency outside [0, 0.5], a thr that is no whole number in [0, 2^32),
        start < 0 or start + n > 2^40) and come out as zeros.  Every sample is a pure function of the row's tables and
        its absolute index: a row made whole and the same row made in pieces with `start` advanced have the same bits.
        Bit-reproducible, row-independent, no synchronisation, graph-capturable after one call at the shape."""
        N, K, NF, P, H, M = check_noise_args(self.device, seed, fir, n, lengths, start, env, env_hop, tones, n_tones, impulse,
                                             out)
        ws = self._grow("noise", int(self.lib.cmgan_noise_workspace_bytes(N)), f"{N} rows are outside what cmgan_noise supports")
        if out is None:
            out = torch.empty(N, K, dtype=torch.float32, device=self.device)
        st = torch.empty(N, dtype=torch.int32, device=self.device)
        if M == 0:
            tones = n_tones = None
        self._call("cmgan_noise", out if K > 0 else None, N, K, out.stride(0) if N > 1 and K > 0 else K, seed, start, lengths, fir,
                   NF, env, P, H, tones, n_tones, M, impulse, st, ws, ws.numel())
        return (out, st) if info else out

    # ---- speed perturbation ---------------------------------------------------------
    def _out_and_info(self, B: int, L: int, N: Optional[int], out: Optional[torch.Tensor], info: bool, n_info: int):
        """What warp and stretch make of checked arguments: (N, out, n_info int32 [B] tensors - None without `info`).  N
        defaults to room for the slowest valid rate, `out` to a new float32 [B, N] tensor."""
        if N is None:
            N = int(self.lib.cmgan_warp_out_len(L, 1.0 / WARP_MAX_RATE))
            if N > 2 ** 31 - 1:
                raise ValueError(f"wav: rows of {L} samples need n_out; the default, {N}, is beyond 2^31 - 1")
        if out is None:
            out = torch.empty(B, N, dtype=torch.float32, device=self.device)
        return N, out, [torch.empty(B, dtype=torch.int32, device=self.device) if info else None for _ in range(n_info)]

    @_on_device
    def warp(self, wav: torch.Tensor, rate: torch.Tensor, n_out: Optional[int] = None, lengths: Optional[torch.Tensor] = None,
             zeros: int = 24, rolloff: float = 0.95, out: Optional[torch.Tensor] = None, info: bool = False):
        """Speed perturbation per row on the GPU (cmgan_warp, include/cmgan_hip.h): every row is resampled by its own rate
        with a Hann-windowed sinc, so that tempo and pitch move together.

        wav float32 [B, L] (rows contiguous, any row stride >= L); rate float64 [B]: input samples per output sample, any
        value in [1 / 4, 4] (> 1 is faster and higher; 1.0001 is a sound card's clock drift); lengths int32 [B] (None:
        every row has L samples; samples from a row's length on are never read).  All on this Engine's device and read by
        the kernel only.  n_out: the output length N; None takes cmgan_warp_out_len(L, 1 / 4), room for the slowest valid
        rate - pass it in real use (cmgan_amd.mixing.warp_len(L, rate) is the length one rate gives).  zeros (4 .. 64)
        zero crossings on either side of the filter's centre; rolloff (0.5 .. 1) the cutoff as a fraction of the lower of
        the two Nyquist rates.  `out` float32 [B, N] is written in place of a new tensor; it may not overlap wav.
        Returns the float32 [B, N] result: row b holds out_len[b] = min(N, #{i : fl(i rate[b]) < lengths[b]}) samples,
        float64 sums with one rounding to float32, then zeros; rate = 1 with rolloff = 1 copies the row bit for bit.
        info=True adds (out_len int32 [B], status int32 [B]): status 1 marks the rows that are invalid (a rate that is
        not a finite number in [1 / 4, 4], a length outside [0, L]) and come out as zeros with out_len 0.
        Bit-reproducible, row-independent, one launch, no workspace, no synchronisation, graph-capturable."""
        B, L, N = check_warp_args(self.device, wav, rate, n_out, lengths, zeros, rolloff, out)
        N, out, (n, st) = self._out_and_info(B, L, N, out, info, 2)
        self._call("cmgan_warp", wav, B, L, wav.stride(0) if B > 1 else L, lengths, rate, int(zeros), float(rolloff), out, N,
                   out.stride(0) if B > 1 else N, n, st)
        return (out, n, st) if info else out

    # ---- tempo and pitch perturbation -------------------------------------------------
    @_on_device
    def stretch(self, wav: torch.Tensor, rate: torch.Tensor, n_out: Optional[int] = None, lengths: Optional[torch.Tensor] = None,
                hop: int = 256, search: int = 160, out: Optional[torch.Tensor] = None, info: bool = False):
        """Tempo perturbation per row on the GPU (cmgan_stretch, include/cmgan_hip.h): every row is time-stretched by its
        own rate with the pitch kept, by WSOLA (waveform-similarity overlap-add): frames of `hop` samples are spliced
        where the waveform continues best, found within +-`search` samples of the nominal position.

        wav float32 [B, L] (rows contiguous, any row stride >= L); rate float64 [B]: input time per output time, any value
        in [1 / 4, 4] (> 1 is faster, the sense of Engine.warp); lengths int32 [B] (None: every row has L samples; samples
        from a row's length on are never read).  All on this Engine's device and read by the kernel only.  n_out: the
        output length N; None takes cmgan_warp_out_len(L, 1 / 4), room for the slowest valid rate - pass it in real use
        (cmgan_amd.mixing.warp_len(L, rate) is the length one rate gives, the same as Engine.warp's).  hop (16 .. 1024)
        and search (0 .. 1024) in samples: the defaults are 16 ms and +-10 ms at 16 kHz, which suits speech.  `out`
        float32 [B, N] is written in place of a new tensor; it may not overlap wav.
        Returns the float32 [B, N] result: row b holds out_len[b] = min(N, #{i : fl(i rate[b]) < lengths[b]}) samples,
        then zeros; a frame that continues the previous one is the input bit for bit, so rate = 1 copies the row.
        info=True returns (y, out_len int32 [B], status int32 [B], pos int32 [B, ceil(N / hop)], searched int32 [B]):
        status 1 marks the rows that are invalid (a rate that is not a finite number in [1 / 4, 4], a length outside
        [0, L]) and come out as zeros with out_len 0; pos holds the input position every frame was taken from (-1 behind a
        row's last frame), searched how many frames were searched.  The positions are exact: a host model finds the same.
        Bit-reproducible, row-independent, one launch (one block per row), no workspace, no synchronisation,
        graph-capturable."""
        B, L, N = check_stretch_args(self.device, wav, rate, n_out, lengths, hop, search, out)
        N, out, (n, st, srch) = self._out_and_info(B, L, N, out, info, 3)
        pos = torch.empty(B, -(-N // int(hop)), dtype=torch.int32, device=self.device) if info else None
        self._call("cmgan_stretch", wav, B, L, wav.stride(0) if B > 1 else L, lengths, rate, int(hop), int(search), out, N,
                   out.stride(0) if B > 1 else N, n, st, pos, srch)
        return (out, n, st, pos, srch) if info else out

    # ---- transmission: codec, packet loss and concealment ---------------------------------
    @_on_device
    def transmit(self, wav: torch.Tensor, lost: torch.Tensor, frame: Optional[int] = None, codec: Optional[torch.Tensor] = None,
                 plc: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None, fs: int = 16000,
                 pmin: Optional[int] = None, pmax: Optional[int] = None, window: Optional[int] = None, fade: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, info: bool = False):
        """A telephone or VoIP link per row on the GPU (cmgan_transmit, include/cmgan_hip.h): a codec, frames that are
        lost, and a receiver that covers the holes by repeating the last pitch period or leaves them as gaps.

        wav float32 [B, L] (rows contiguous, any row stride >= L); lost uint8 [B, n_frames] with n_frames >= ceil(L /
        frame): non-zero where a frame of `frame` samples is lost (cmgan_amd.mixing.TransmissionSampler draws bursty
        patterns); codec int32 [B]: 0 none, 1 16-bit PCM, 2 G.711 mu-law, 3 G.711 A-law (TRANSMIT_CODECS; None: none); plc
        int32 [B]: 1 conceals a run of lost frames, 0 leaves zeros (None: conceal); lengths int32 [B] (None: every row
        has L samples; samples from a row's length on are never read and come out as zeros, and neither are the table
        columns behind its last frame).  All on this Engine's device and read by the kernels only.  The host values
        default from `fs`: frame fs / 50 (20 ms), the lag range pmin = fs / 200 .. pmax = 3 fs / 200 (66 .. 200 Hz), the
        matching window fs / 50 and the fade unit fade = fs / 100: a concealed run keeps its level for `fade` samples,
        then falls by 20 % per `fade` and is silent from 6 `fade` on (60 ms).  `out` float32 [B, L] is written in place of
        a new tensor; out=wav runs in place.  Returns the float32 [B, L] result: float64 arithmetic with one rounding to
        float32 per concealed sample; codec 0 with no lost frame copies the row bit for bit.  info=True adds (status int32
        [B], lag int32 [B, n_frames]): status 1 marks the rows that are invalid (a codec outside 0 .. 3, a plc outside 0
        .. 1, a length outside [0, L]) and come out as zeros; lag holds the pitch lag at the frame that starts a concealed
        run, 0 at a row's other frames and -1 behind its last (a view of a table as wide as lost's rows are apart, when
        lost is a column slice of a wider one).  The lags are exact: a host model finds the same.
        Bit-reproducible, row-independent, two launches (the second one block per row), no workspace, no synchronisation,
        graph-capturable."""
        B, L, F, pmin, pmax, W, A = check_transmit_args(self.device, wav, lost, frame, codec, plc, lengths, fs, pmin, pmax,
                                                         window, fade, out)
        if codec is None:
            codec = torch.zeros(B, dtype=torch.int32, device=self.device)
        if plc is None:
            plc = torch.ones(B, dtype=torch.int32, device=self.device)
        if out is None:
            out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        st = torch.empty(B, dtype=torch.int32, device=self.device) if info else None
        # the kernels know ONE leading dimension for both tables, lost's: lag is allocated as wide as lost's rows are apart
        # (a column slice of a wider table included) and returned as its first n_frames columns
        n_frames = lost.size(1)
        ldl = lost.stride(0) if B > 1 else n_frames
        lag = torch.empty(B, ldl, dtype=torch.int32, device=self.device) if info else None
        self._call("cmgan_transmit", wav, B, L, wav.stride(0) if B > 1 else L, lengths, lost, ldl, codec, plc, F, pmin, pmax,
                   W, A, out, out.stride(0) if B > 1 else L, st, lag)
        return (out, st, lag[:, :n_frames]) if info else out

    # ---- suppression: the device's own noise suppressor, and the classical baseline -----------
    @_on_device
    def suppress(self, wav: torch.Tensor, table: torch.Tensor, n_fft: int = 512, lengths: Optional[torch.Tensor] = None,
                 key: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, info: bool = False):
        """A single-channel noise suppressor per row on the GPU (cmgan_suppress, include/cmgan_hip.h): a short-time spectral
        gain from a minimum-tracking noise estimate and the decision-directed a-priori SNR - the Wiener rule, power spectral
        subtraction or Ephraim and Malah's log-MMSE rule.

        wav float32 [B, L] (rows contiguous, any row stride >= L); table float64 [B, 7] = (rule, a_dd, a_n, D, bias, g_min,
        xi_min) per row (cmgan_amd.mixing.suppress_params makes it from audio units; rule 0 copies the row bit for bit);
        n_fft 256, 512 or 1024: frames of n_fft samples under a square-root Hann window every n_fft / 2; lengths int32 [B]
        (None: every row has L samples; samples from a row's length on are never read, and come out as zeros); key float32
        [B, L]: the signal whose spectrum drives the gains (None: wav itself).  All on this Engine's device and read by the
        kernels only.  `out` float32 [B, L] is written in place of a new tensor; out=wav runs in place, out=key is allowed,
        any other overlap of out with wav or key is a ValueError.  Returns the float32 [B, L] result: float64 arithmetic
        with one rounding to float32.  info=True adds (status, gain): int32 [B], 1 for the rows that are invalid (a table
        entry that is not finite or out of range, a rule or D that is no integer, a length outside [0, L]) and come out as
        zeros, and float64 [B, T, n_fft / 2 + 1] with T = suppress_frames(L, n_fft), the gain of every frame and bin (1 at
        rule 0, 0 behind a row's last frame).  Bit-reproducible, row-independent, three launches, no synchronisation,
        graph-capturable after one call at the shape."""
        B, L = check_suppress_args(self.device, wav, table, n_fft, lengths, key, out)
        ws = self._grow("suppress", int(self.lib.cmgan_suppress_workspace_bytes(B, L, int(n_fft))),
                        f"[{B}, {L}] at n_fft = {n_fft} is outside what cmgan_suppress supports")
        if out is None:
            out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        st = torch.empty(B, dtype=torch.int32, device=self.device) if info else None
        gain = None
        if info:
            gain = torch.empty(B, suppress_frames(L, int(n_fft)), int(n_fft) // 2 + 1, dtype=torch.float64, device=self.device)
        self._call("cmgan_suppress", wav, B, L, wav.stride(0) if B > 1 else L, key,
                   0 if key is None else (key.stride(0) if B > 1 else L), lengths, table, int(n_fft), out,
                   out.stride(0) if B > 1 else L, st, gain, ws, ws.numel())
        return (out, st, gain) if info else out

    # ---- auxiliary losses: multi-resolution STFT loss and negative SI-SDR, with their gradient ----------
    def _aux_workspace(self, B: int, L: int, n_ffts) -> torch.Tensor:
        arr = (ctypes.c_int * len(n_ffts))(*n_ffts)
        return self._grow("aux_loss", int(self.lib.cmgan_aux_loss_workspace_bytes(self._h, B, L, len(n_ffts), arr)),
                          f"[{B}, {L}] at n_ffts = {tuple(n_ffts)} is outside what cmgan_aux_loss supports")

    @_on_device
    def aux_loss(self, est: torch.Tensor, ref: torch.Tensor, n_ffts=(512, 1024, 2048), w_mr: float = 1.0, w_si: float = 0.0,
                 grad: bool = True) -> AuxLossOut:
        """The multi-resolution STFT loss and negative SI-SDR of an estimate against a reference, with the gradient with
        respect to the estimate (cmgan_aux_loss, include/cmgan_hip.h, "Auxiliary losses", states every formula).

        est, ref float32 [B, L], contiguous, on this Engine's device; n_ffts 1 to 4 distinct window lengths from (256, 512,
        1024, 2048), hop n / 4, periodic Hann, centred frames with reflect padding (L > max(n_ffts) / 2); w_mr, w_si >= 0
        weigh the batch MEANS of the two terms: total = sum_b (w_mr / B) MR_b - (w_si / B) SISDR_b, so a row's outputs do
        not depend on its neighbours.  Returns AuxLossOut(total float32 [3], rows float64 [B, 2 R + 1], grad float32 [B, L])
        of device tensors; rows holds (spectral convergence, log-magnitude L1) per resolution and the row's SI-SDR in dB
        whatever the weights are, so grad=False (grad is then None, total and rows keep their bits) is a scorer.  float64
        arithmetic with one rounding, bit-reproducible, row-independent, no synchronisation; graph-capturable after one
        call at the shape.  The gradient is never formed over est or ref."""
        B, L, res, w_mr, w_si = check_aux_loss_args(self.device, est, ref, n_ffts, w_mr, w_si)
        ws = self._aux_workspace(B, L, res)
        rows = torch.empty(B, 2 * len(res) + 1, dtype=torch.float64, device=self.device)
        total = torch.empty(3, dtype=torch.float32, device=self.device)
        g = torch.empty(B, L, dtype=torch.float32, device=self.device) if grad else None
        self._call("cmgan_aux_loss", est, ref, B, L, len(res), (ctypes.c_int * len(res))(*res), w_mr / B, w_si / B, rows, total,
                   g, ws, ws.numel())
        return AuxLossOut(total, rows, g)

    # ---- intelligibility: negative STOI / ESTOI as a loss term with its gradient, ESTOI as a score ----------
    def _stoi_workspace(self, B: int, L: int) -> torch.Tensor:
        return self._grow("stoi_loss", int(self.lib.cmgan_stoi_loss_workspace_bytes(self._h, B, L, 16000)),
                          f"[{B}, {L}] is outside what cmgan_stoi_loss supports: 16 kHz rows of at least {STOI_MIN_L} samples")

    @_on_device
    def stoi_loss(self, est: torch.Tensor, ref: torch.Tensor, weight: float = 1.0, extended: bool = False,
                  grad: bool = True) -> StoiLossOut:
        """Negative STOI (extended=True: ESTOI) of a 16 kHz estimate against a reference as a loss, with the gradient with
        respect to the estimate (cmgan_stoi_loss, include/cmgan_hip.h, "Intelligibility loss", states every formula).

        est, ref float32 [B, L], contiguous, on this Engine's device, L >= 6554 (31 frames at 10 kHz).  total = sum over the
        rows of -(weight / B) STOI_b, so a row's outputs do not depend on its neighbours.  The forward is Engine.metrics'
        STOI column sum for sum; the silent-frame decision is made from `ref` alone and is a constant of the gradient.
        Returns StoiLossOut(total float32 [1], rows float64 [B, 2] = (value, kept frames), status int32 [B], grad float32
        [B, L]) of device tensors.  A row whose reference keeps fewer than 31 frames (status bit 0) or whose value is not
        finite (bit 1: an all-zero estimate) has NaN in rows, is left out of total and has a gradient of exact zeros.
        grad=False: grad is None, the rest keeps its bits.  float64 arithmetic with one rounding, bit-reproducible,
        row-independent, no synchronisation; graph-capturable after one call at the shape.  The gradient is never formed
        over est or ref."""
        B, L, weight, extended = check_stoi_loss_args(self.device, est, ref, weight, extended)
        ws = self._stoi_workspace(B, L)
        rows = torch.empty(B, 2, dtype=torch.float64, device=self.device)
        total = torch.empty(1, dtype=torch.float32, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        g = torch.empty(B, L, dtype=torch.float32, device=self.device) if grad else None
        self._call("cmgan_stoi_loss", est, ref, B, L, 16000, 1 if extended else 0, weight / B, rows, total, status, g, ws,
                   ws.numel())
        return StoiLossOut(total, rows, status, g)

    def estoi(self, clean: torch.Tensor, enhanced: torch.Tensor) -> torch.Tensor:
        """ESTOI (Jensen and Taal 2016) of every row of a 16 kHz batch: float64 [B] on the device, NaN where the row has a
        status (Engine.stoi_loss).  clean, enhanced float32 [B, L] as Engine.stoi_loss takes them; the values alone, no
        gradient is formed."""
        return self.stoi_loss(enhanced, clean, 1.0, True, grad=False).rows[:, 0].contiguous()

    # ---- phase: the anti-wrapping terms of MP-SENet on the emitted spectrum, with their gradient ----------
    def _phase_workspace(self, B: int, T: int) -> torch.Tensor:
        return self._grow("phase_loss", int(self.lib.cmgan_phase_loss_workspace_bytes(self._h, B, T)),
                          f"[{B}, {T}] is outside what cmgan_phase_loss supports: 1 .. 65535 rows of 1 .. {PHASE_MAX_T} frames")

    @_on_device
    def phase_loss(self, est_real: torch.Tensor, est_imag: torch.Tensor, clean_spec: torch.Tensor, w_ip: float = 1.0,
                   w_gd: float = 1.0, w_iaf: float = 1.0, floor: float = 0.0, grad: bool = True) -> PhaseLossOut:
        """The anti-wrapping instantaneous-phase, group-delay and instantaneous-angular-frequency terms (MP-SENet) of the
        spectrum est_real + i est_imag against clean_spec, with the gradient with respect to est_real and est_imag
        (cmgan_phase_loss, include/cmgan_hip.h, "Phase loss", states every formula and order of summation).

        est_real, est_imag float32 [B, 1, T, F] (or [B, T, F]), clean_spec float32 [B, 2, T, F], contiguous, on this Engine's
        device, F the Engine's.  A cell whose estimate or clean magnitude is 0 or below `floor`, or that holds a non-finite
        value, is void and takes its terms with it; each term is the mean over the row's own non-void terms, and w_ip,
        w_gd, w_iaf >= 0 weigh the batch MEANS: total[0] = sum_b sum_i (w_i / B) value_i, so a row's outputs do not depend
        on its neighbours.  Returns PhaseLossOut(total float32 [4], rows float64 [B, 3], counts int32 [B, 3], status int32
        [B], g_real, g_imag float32 of est_real's shape) of device tensors.  A term without a non-void term (T = 1 has no
        IAF pair) has value 0, no gradient and its bit in status.  grad=False: g_real and g_imag are None, the rest keeps
        its bits.  float64 arithmetic with one rounding, bit-reproducible, row-independent, no synchronisation;
        graph-capturable after one call at the shape.  The gradient is never formed over an input."""
        B, T, w_ip, w_gd, w_iaf, floor = check_phase_loss_args(self.device, self.F, est_real, est_imag, clean_spec, w_ip, w_gd,
                                                               w_iaf, floor)
        ws = self._phase_workspace(B, T)
        rows = torch.empty(B, 3, dtype=torch.float64, device=self.device)
        counts = torch.empty(B, 3, dtype=torch.int32, device=self.device)
        total = torch.empty(4, dtype=torch.float32, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        g_real = torch.empty_like(est_real) if grad else None
        g_imag = torch.empty_like(est_imag) if grad else None
        self._call("cmgan_phase_loss", est_real, est_imag, clean_spec, B, T, w_ip / B, w_gd / B, w_iaf / B, floor, rows, counts,
                   total, status, g_real, g_imag, ws, ws.numel())
        return PhaseLossOut(total, rows, counts, status, g_real, g_imag)

    @_on_device
    def pitch_shift(self, wav: torch.Tensor, factor: torch.Tensor, n_out: Optional[int] = None, hop: int = 256,
                    search: int = 160, zeros: int = 24, rolloff: float = 0.95):
        """Pitch perturbation per row on the GPU without a tempo change: Engine.stretch at rate 1 / factor, which makes
        the row `factor` times as long at its own pitch, then Engine.warp at rate `factor`, which brings it back to its
        length and multiplies every frequency by `factor`.

        wav float32 [B, L]; factor float64 [B] on this Engine's device, a frequency ratio in [1 / 2, 2] (2^(s / 12) for s
        semitones), read on the device only.  n_out: the output length (None: L).  hop / search are Engine.stretch's,
        zeros / rolloff Engine.warp's.  Returns float32 [B, n_out].  A row holds min(n_out, M2) samples and zeros after
        them, M2 = warp_len(warp_len(L, 1 / factor), factor): L up to the two roundings of the length, and the pitch is
        `factor` times the input's up to the same.  A row whose factor is not a finite number in [1 / 2, 2] comes out as
        zeros.  factor = 1 gives Engine.warp's output at rate 1 (the stretch is then a copy).  The stretch is WSOLA tuned to
        speech (frames of 16 ms, splices searched within +-10 ms at the defaults): it is not meant for music, whose
        polyphony has no single period to splice at.  Two launches and an intermediate of warp_len(L, 1 / 2) samples per
        row; no synchronisation."""
        B, L = check_pitch_args(self.device, wav, factor, n_out, hop, search, zeros, rolloff)
        ok = (factor >= PITCH_FACTOR[0]) & (factor <= PITCH_FACTOR[1])                      # a NaN: False
        f = torch.where(ok, factor, torch.full_like(factor, float("nan")))                   # (an invalid row of both calls)
        N1 = int(self.lib.cmgan_warp_out_len(L, PITCH_FACTOR[0]))
        if N1 > 2 ** 31 - 1:
            raise ValueError(f"wav: rows of {L} samples are too long: the stretched batch would need {N1} samples per row")
        long, n1, _, _, _ = self.stretch(wav, 1.0 / f, N1, hop=hop, search=search, info=True)
        return self.warp(long, f, L if n_out is None else n_out, n1, zeros, rolloff)

    # ---- diagnostics ---------------------------------------------------------------
    @_on_device
    def selftest_mfma(self) -> float:
        err = ctypes.c_float()
        native_call(self, "cmgan_selftest_mfma", ctypes.byref(err))
        return float(err.value)

    @_on_device
    def selftest_mfma_x3(self) -> float:
        err = ctypes.c_float()
        native_call(self, "cmgan_selftest_mfma_x3", ctypes.byref(err))
        return float(err.value)

    def mask_head_weights(self):
        """The mask decoder's folded sub_pixel x conv_1 table as the library derived it (cmgan_mask_head_weights):
        (G [3, 64, 2, 2], g0 [2, 2])."""
        out = np.zeros(776, dtype=np.float32)
        native_call(self, "cmgan_mask_head_weights", out.ctypes.data_as(ctypes.c_void_p))
        return out[:768].reshape(3, 64, 2, 2).copy(), out[768:].reshape(2, 4)[:, :2].copy()

    @_on_device
    def mask_head(self, y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
        """The mask decoder's head alone (cmgan_mask_head_forward): y [B, T, Fe, 64], scale / shift [B, 64] ->
        dm [B, T, 2 Fe, 4]."""
        y = tensor_arg(y, "y", torch.float32, self.device, "[B, T, Fe, 64]", lambda t: t.dim() == 4 and t.size(3) == 64)
        B, T, Fe = (int(v) for v in y.shape[:3])
        ok = lambda t: tuple(t.shape) == (B, 64)
        scale = tensor_arg(scale, "scale", torch.float32, self.device, "[B, 64]", ok)
        shift = tensor_arg(shift, "shift", torch.float32, self.device, "[B, 64]", ok)
        dm = torch.empty(B, T, 2 * Fe, 4, dtype=torch.float32, device=self.device)
        self._call("cmgan_mask_head_forward", y, scale, shift, B, T, Fe, dm)
        return dm

    def release_workspaces(self):
        """Drop the inference workspaces and every captured graph that points into them (they are re-created on demand):
        ~6 GB each at 32 x 2 s.  bench.py calls this before its training leg."""
        self._graphs.clear()
        self._row_graphs.clear()
        self._stream_slots.clear()
        self._wss.clear()

    def set_profiling(self, on: bool):
        native_call(self, "cmgan_set_profiling", 1 if on else 0)

    def profile(self):
        """[(kernel name, ms)] of the most recent forward (profiling must be on)."""
        cap = 1024
        buf = (KernelTime * cap)()
        n = self.lib.cmgan_profile_read(self._h, buf, cap)
        return [(buf[i].name.decode(), float(buf[i].ms)) for i in range(n)]
