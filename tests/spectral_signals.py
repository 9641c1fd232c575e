"""Test signals for the STFT / ISTFT kernels (tests/test_gpu_spectral.py): clips and spectra whose edges are where an
index error shows - a 60 dB gain step at every hop, asymmetric transients in the first and last 200 samples (a wrong
reflection at either end changes the result), a stretch of digital silence longer than n_fft and a segment at 1e-19
amplitude - and spectra that no real signal produces (non-zero imaginary DC and Nyquist bins).  Every row of a batch
has its own content, so a row mix-up shows."""
import numpy as np
import torch


def clip(L: int, seed: int, n_fft: int = 400, hop: int = 100) -> torch.Tensor:
    """One float32 row of L samples."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal(L)
    steps = np.array([1.0, 1e-3, 1e-1, 1e-2])                  # 60 dB apart at most, every hop
    x *= steps[(np.arange(L) // hop + seed) % 4]
    n = np.arange(L, dtype=np.float64)
    a = 3 + seed % 5                                         # one-sided bursts, not symmetric about either end
    x += 5.0 * np.exp(-np.maximum(n - a, 0) / 17.0) * np.cos(0.7 * n) * (n >= a)
    e = n - (L - 131)
    x += 4.0 * (np.clip(e, 0, None) / 131.0) ** 2 * np.sin(1.3 * n) * (e >= 0)
    if L >= 3 * n_fft + 4 * hop:                             # digital silence, n_fft + 2 hops long
        s0 = L // 3
        x[s0:s0 + n_fft + 2 * hop] = 0.0
    if L >= 6 * n_fft:                                       # a segment at 1e-19 amplitude
        s1 = (2 * L) // 3
        x[s1:s1 + n_fft + hop] = 1e-19 * g.standard_normal(n_fft + hop)
    return torch.from_numpy(x * (1.0 + seed % 3)).float()


def clips(B: int, L: int, seed: int, n_fft: int = 400, hop: int = 100) -> torch.Tensor:
    return torch.stack([clip(L, seed + 7919 * b, n_fft, hop) for b in range(B)])


def spectra(B: int, T: int, F: int, seed: int):
    """Compressed (re, im) [B,1,T,F] in float32: Gaussian bins (imaginary DC / Nyquist included), the frame gain stepping
    between 1 and 10^-0.9 (60 dB once uncompressed), four all-zero frames and four frames at 1e-5 (~1e-17 uncompressed)."""
    g = torch.Generator().manual_seed(seed)
    re, im = torch.randn(B, 1, T, F, generator=g), torch.randn(B, 1, T, F, generator=g)
    gain = torch.tensor([1.0, 10 ** -0.9])[(torch.arange(T) + seed) % 2]
    gain = gain * (1.0 + torch.arange(B)[:, None] % 3)
    if T >= 16:
        gain[:, T // 3:T // 3 + 4] = 0.0
        gain[:, (2 * T) // 3:(2 * T) // 3 + 4] = 1e-5
    return re * gain[:, None, :, None], im * gain[:, None, :, None]
