"""CPU side of the GPU metric kernels (cmgan_amd/csrc/metrics.hip): the tables they build, exported through
cmgan_metrics_table from the same C++ code, against scipy and cmgan_amd.metrics; numpy models of the two kernel
algorithms that differ in form from the host module (radix-select trimmed mean, gather-form STOI compaction); and the
argument errors that need no GPU."""
import ctypes
import math

import numpy as np
import pytest
from scipy import signal as sig

from cmgan_amd import _lib
from cmgan_amd import metrics as M
from metrics_signals import CASES, pair

TOL = 1e-13


def table(fs, which):
    lib = _lib.load()
    n = lib.cmgan_metrics_table(fs, which, None, 0)
    assert n > 0, n
    out = np.full(n, np.nan)
    assert lib.cmgan_metrics_table(fs, which, out.ctypes.data_as(ctypes.c_void_p), n) == n
    return out


@pytest.mark.parametrize("fs,up,down", [(16000, 5, 8), (8000, 5, 4)])
def test_resample_fir_matches_scipy_construction(fs, up, down):
    """resample_poly(x, 10000, fs): firwin(2 * 10 * max + 1, 1 / max, ('kaiser', 5.0)) * up, zero pre-pad of
    down - half_len % down taps (scipy/signal/_signaltools.py)."""
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = sig.firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    want = np.concatenate([np.zeros(down - half_len % down), h])
    got = table(fs, 4)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= TOL


@pytest.mark.parametrize("fs", [16000, 8000])
def test_wss_bank_and_taper_match_the_host_module(fs):
    win, _ = M._win_hop(fs)
    n = np.arange(1, win + 1)
    assert np.max(np.abs(table(fs, 0) - 0.5 * (1.0 - np.cos(2.0 * math.pi * n / (win + 1))))) <= TOL
    half = int(2 ** math.ceil(math.log2(2 * win))) // 2
    bins = np.arange(half)
    f0 = np.floor(M._CB_CENTRE / (fs / 2) * half)[:, None]
    bw = (M._CB_WIDTH / (fs / 2) * half)[:, None]
    gain = (np.log(M._CB_WIDTH[0]) - np.log(M._CB_WIDTH))[:, None]
    bank = np.exp(-11.0 * ((bins[None, :] - f0) / bw) ** 2 + gain)
    bank[bank <= math.exp(-30.0 / (2.0 * 2.303))] = 0.0
    t = table(fs, 1)
    dense = np.zeros_like(bank)
    for b in range(25):
        first, count = int(t[b]), int(t[25 + b])
        assert 0 < count < 64
        dense[b, first:first + count] = t[50 + 64 * b: 50 + 64 * b + count]
    assert np.max(np.abs(dense - bank)) <= TOL


def test_stoi_bands_and_window_match_the_host_module():
    t = table(16000, 2)
    assert np.array_equal(t, table(8000, 2))              # STOI always runs at 10 kHz
    want = M._third_octave_bands(10000, 512, 15, 150.0)
    nb = int(t[0])
    got = np.zeros((nb, 257))
    for k in range(nb):
        got[k, int(t[1 + 2 * k]):int(t[2 + 2 * k])] = 1.0
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.max(np.abs(table(16000, 3) - M._hann_inner(256))) <= TOL


# ------------------------------------------------------------------ numpy models of the kernels' algorithms
def _okey(v):
    """metrics.hip okey(): order-preserving uint64 image of float64, NaN last."""
    u = np.asarray(v, dtype=np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)) == 1
    k = np.where(neg, ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(v), np.uint64(2 ** 64 - 1), k)


def radix_trimmed_mean(v, k):
    """metrics.hip trimmed_mean(): 4-bit radix select of the k-th smallest key, then one masked sum."""
    keys = _okey(v)
    prefix, mask, krem = 0, 0, k
    for shift in range(60, -1, -4):
        live = (keys & np.uint64(mask)) == np.uint64(prefix)
        digit = ((keys >> np.uint64(shift)) & np.uint64(15)).astype(np.int64)
        counts = np.bincount(digit[live], minlength=16)
        d = 0
        while d < 15 and krem > counts[d]:
            krem -= counts[d]
            d += 1
        prefix |= d << shift
        mask |= 15 << shift
    below = keys < np.uint64(prefix)
    kth = v[np.flatnonzero(keys == np.uint64(prefix))[0]]
    return (np.sum(v[below]) + (k - np.count_nonzero(below)) * kth) / k


def gather_compaction(x, y, dyn, n, hop):
    """metrics.hip keep mask + exclusive scan + overlap-add written as a gather (each output sample reads at most two
    kept frames, earlier frame first - the order np.add.at adds them in)."""
    starts = np.arange(0, x.size - n, hop)
    w = M._hann_inner(n)
    idx = (starts[:, None] - 1 + np.arange(n)[None, :]) % x.size
    level = 20.0 * np.log10(np.sqrt(np.sum((x[idx] * w) ** 2, axis=1)) / math.sqrt(n))
    keep = ((level - level.max()) + dyn) > 0
    pos = np.cumsum(keep) - keep                             # exclusive scan
    src = np.zeros(int(keep.sum()), dtype=np.int64)
    src[pos[keep]] = np.flatnonzero(keep)
    K = src.size
    out = []
    for s in (x, y):
        t = np.arange((K - 1) * hop + n)
        p = t // hop
        acc = np.zeros(t.size)
        for q in (p - 1, p):
            ok = (q >= 0) & (q < K)
            o = t[ok] - q[ok] * hop
            acc[ok] = acc[ok] + s[src[q[ok]] * hop + o] * w[o]
        out.append(acc)
    return out


@pytest.mark.parametrize("fs,n,seed", CASES)
def test_radix_select_trimmed_mean_equals_sort_and_mean(fs, n, seed):
    clean, enh = pair(fs, n, seed)
    for v in (M.wss(clean, enh, fs), M.llr(clean, enh, fs)):
        k = round(v.size * 0.95)
        want = float(np.mean(np.sort(v)[:k]))
        assert abs(radix_trimmed_mean(v, k) - want) <= 1e-13 * abs(want)
    # ties, negatives, signed zeros and a NaN (sorted last, like np.sort)
    v = np.array([3.0, -1.0, 3.0, 0.0, -0.0, np.nan, 2.5, -7.25, 3.0, 1e-300])
    for k in range(1, v.size + 1):
        want = float(np.mean(np.sort(v)[:k]))
        got = radix_trimmed_mean(v, k)
        assert (math.isnan(want) and math.isnan(got)) or abs(got - want) <= 1e-15 * max(1.0, abs(want)), k


@pytest.mark.parametrize("fs,n,seed", CASES)
def test_gather_form_stoi_compaction_equals_the_host(fs, n, seed):
    clean, enh = pair(fs, n, seed)
    x, y = sig.resample_poly(clean, 10000, fs), sig.resample_poly(enh, 10000, fs)
    want = M._drop_silent_frames(x, y, 40.0, 256, 128)
    got = gather_compaction(x, y, 40.0, 256, 128)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


# ------------------------------------------------------------------ argument errors without a GPU
def test_metric_argument_errors_without_gpu():
    lib = _lib.load()
    assert lib.cmgan_metrics_table(44100, 0, None, 0) == -3                 # CMGAN_E_UNSUPPORTED
    assert lib.cmgan_metrics_table(48000, 4, None, 0) == -3
    assert lib.cmgan_metrics_table(16000, 9, None, 0) == -1                 # CMGAN_E_BADARG
    small = np.zeros(4)
    assert lib.cmgan_metrics_table(16000, 0, small.ctypes.data_as(ctypes.c_void_p), small.size) == -1
    assert lib.cmgan_metrics_workspace_bytes(None, 1, 479, 16000) == 0      # L < win
    assert lib.cmgan_metrics_workspace_bytes(None, 1, 6553, 16000) == 0     # no 30-frame STOI window
    assert lib.cmgan_metrics_workspace_bytes(None, 1, 6554, 16000) > 0
    assert lib.cmgan_metrics_workspace_bytes(None, 1, 32000, 44100) == 0
    assert lib.cmgan_metrics_workspace_bytes(None, 0, 32000, 16000) == 0
    assert lib.cmgan_metrics(None, None, None, 1, 32000, 16000, None, 0.0, None, None, None, 0, None) == -1
