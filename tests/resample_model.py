"""Numpy restatement of the resampling contract (include/cmgan_hip.h, "Sample-rate conversion"): the geometry
formulas, scipy's tap construction, and the output sum written as the plain loop the kernel implements.  float64
throughout; tests/test_resample_host.py holds it to scipy.signal.resample_poly."""
import math

import numpy as np
from scipy import signal as sig

#: the rate pairs every resampling test covers
PAIRS = [(44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000), (8000, 16000), (22050, 16000), (32000, 16000),
         (11025, 16000), (24000, 16000), (44100, 48000), (96000, 16000)]


def geometry(fs_in, fs_out):
    """(up, down, n_taps incl. the pre-pad, pre_remove)."""
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    half_len = 10 * max(up, down)
    pre = down - half_len % down
    return up, down, pre + 2 * half_len + 1, (half_len + pre) // down


def out_len(fs_in, fs_out, n_in):
    up, down, _, _ = geometry(fs_in, fs_out)
    return -(-n_in * up // down)


def taps(fs_in, fs_out):
    """scipy's construction (scipy/signal/_signaltools.py: resample_poly): firwin * up behind `pre` zeros."""
    up, down, n_taps, _ = geometry(fs_in, fs_out)
    m = max(up, down)
    h = sig.firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    return np.concatenate([np.zeros(n_taps - h.size), h])


def resample(x, fs_in, fs_out, n0=0, n_out=None, pos_in=0):
    """y[n] = sum_i x[i] h[(n + pre_remove) down - i up] for n in [n0, n0 + n_out), taps added in ascending tap index.
    `x` holds samples [pos_in, pos_in + len(x)) of the signal; the others count as zero."""
    x = np.asarray(x, dtype=np.float64)
    if fs_in == fs_out:
        full = np.zeros(n0 + (x.size if n_out is None else n_out))
        full[pos_in:pos_in + x.size] = x[:max(full.size - pos_in, 0)]
        return full[n0:]
    up, down, n_taps, pre_remove = geometry(fs_in, fs_out)
    h = taps(fs_in, fs_out)
    if n_out is None:
        n_out = out_len(fs_in, fs_out, pos_in + x.size) - n0
    y = np.zeros(n_out)
    for o in range(n_out):
        pos = (n0 + o + pre_remove) * down
        i_hi = pos // up
        i_lo = max(-(-(pos - (n_taps - 1)) // up), 0)
        acc = 0.0
        for i in range(i_hi, i_lo - 1, -1):                    # descending input = ascending tap index
            if pos_in <= i < pos_in + x.size:
                acc += x[i - pos_in] * h[pos - i * up]
        y[o] = acc
    return y


def resample_fast(x, fs_in, fs_out):
    """The same sum, vectorised per phase (for the long signals of the GPU tests' expectations scipy itself is used;
    this form only checks the loop above on longer inputs)."""
    x = np.asarray(x, dtype=np.float64)
    up, down, n_taps, pre_remove = geometry(fs_in, fs_out)
    h = taps(fs_in, fs_out)
    n = np.arange(out_len(fs_in, fs_out, x.size))
    pos = (n + pre_remove) * down
    i_hi, p = pos // up, pos % up
    T = -(-n_taps // up)
    hp = np.zeros((up, T))
    for q in range(up):
        col = h[q::up]
        hp[q, :col.size] = col
    y = np.zeros(n.size)
    for j in range(T):
        i = i_hi - j
        ok = (i >= 0) & (i < x.size)
        y[ok] += x[i[ok]] * hp[p[ok], j]
    return y
