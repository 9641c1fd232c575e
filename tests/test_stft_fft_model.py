"""Lane-level numpy model of stft_fft400_kernel / istft_fft400_kernel (cmgan_amd/csrc/stft.hip): the 400-point real DFT as a
16 x 25 factorisation - pass 1 = 25-point DFTs (5 x 5) of x[16 m + r] per residue r, twiddle W400^{r k'}, pass 2 = 16-point DFTs
(4 x 4) per channel k' = 0..12, bins above N/2 taken as conjugates of the missing channels.  The model uses the kernel's own
butterflies, index maps and table layouts (tools/gen_fft_tables.py) and must reproduce numpy's rfft / irfft; it also checks
that every one of the 201 bins is produced exactly once."""
import numpy as np

N = 400
W = lambda n, e: np.exp(-2j * np.pi * (e % n) / n)
C1, C2, S1, S2 = np.cos(2 * np.pi / 5), np.cos(4 * np.pi / 5), np.sin(2 * np.pi / 5), np.sin(4 * np.pi / 5)


def dft5(x, inv=False):
    rot = (lambda z: 1j * z) if inv else (lambda z: -1j * z)
    t1, t2, t3, t4 = x[1] + x[4], x[2] + x[3], x[1] - x[4], x[2] - x[3]
    a1, a2 = x[0] + C1 * t1 + C2 * t2, x[0] + C2 * t1 + C1 * t2
    r1, r2 = rot(S1 * t3 + S2 * t4), rot(S2 * t3 - S1 * t4)
    return np.array([x[0] + t1 + t2, a1 + r1, a2 + r2, a2 - r2, a1 - r1])


def dft4(x, inv=False):
    rot = (lambda z: 1j * z) if inv else (lambda z: -1j * z)
    t0, t1, t2, t3 = x[0] + x[2], x[0] - x[2], x[1] + x[3], x[1] - x[3]
    return np.array([t0 + t2, t1 + rot(t3), t0 - t2, t1 - rot(t3)])


def forward(x):
    H = np.zeros((16, 13), complex)
    for r in range(16):                                       # pass 1: lane r
        v = x[16 * np.arange(25) + r].astype(complex)
        C = np.array([dft5(v[5 * np.arange(5) + b]) for b in range(5)])          # C[b][c]
        for c in range(5):
            y = dft5(np.array([C[b][c] * W(25, b * c) for b in range(5)]))       # y[d] = G[c + 5 d]
            for d in range(3):
                if c + 5 * d < 13:
                    H[r][c + 5 * d] = y[d] * W(400, r * (c + 5 * d))
    X, cnt = np.zeros(201, complex), np.zeros(201, int)
    for kp in range(13):                                      # pass 2: lane k'
        inner = np.array([dft4(H[4 * np.arange(4) + q, kp]) for q in range(4)])  # inner[q][s]
        for s in range(4):
            y = dft4(np.array([inner[q][s] * W(16, q * s) for q in range(4)]))   # y[u] = Y[s + 4 u]
            for u in range(4):
                k = kp + 25 * (s + 4 * u)
                if k <= 200:
                    X[k] = y[u]; cnt[k] += 1
                elif kp != 0:
                    X[400 - k] = np.conj(y[u]); cnt[400 - k] += 1
    return X, cnt


def inverse(Y):
    """Y[0..200] -> x[0..399] = irfft(Y, 400) by the mirrored passes (imaginary parts of DC / Nyquist ignored)."""
    Y = Y.copy()
    Y[0], Y[200] = Y[0].real, Y[200].real
    Hh = np.zeros((16, 13), complex)
    for kp in range(13):                                      # pass A: lane k': inverse 16-point DFT over k1
        ch = np.zeros(16, complex)
        for k1 in range(16):
            k = kp + 25 * k1
            ch[k1] = Y[k] if k <= 200 else np.conj(Y[400 - k])
        inner = np.array([dft4(ch[4 * np.arange(4) + q], inv=True) for q in range(4)])          # over p: k1 = 4 p + q
        for s in range(4):
            y = dft4(np.array([inner[q][s] * np.conj(W(16, q * s)) for q in range(4)]), inv=True)   # y[u] = h[s + 4 u]
            for u in range(4):
                r = s + 4 * u
                Hh[r][kp] = y[u] * np.conj(W(400, r * kp))
    x = np.zeros(400)
    for r in range(16):                                       # pass B: lane r: inverse 25-point DFT, Hermitian input
        full = np.zeros(25, complex)
        full[:13] = Hh[r]
        full[13:] = np.conj(Hh[r][12:0:-1])
        C = np.array([dft5(full[5 * np.arange(5) + b], inv=True) for b in range(5)])           # k' = 5 a + b
        for c in range(5):
            y = dft5(np.array([C[b][c] * np.conj(W(25, b * c)) for b in range(5)]), inv=True)  # y[d] -> m = c + 5 d
            for d in range(5):
                x[16 * (c + 5 * d) + r] = y[d].real / N
    return x


def test_forward_passes_reproduce_rfft_and_cover_every_bin_once():
    rng = np.random.default_rng(0)
    for _ in range(3):
        x = rng.standard_normal(N)
        X, cnt = forward(x)
        assert (cnt == 1).all()
        ref = np.fft.rfft(x)
        assert np.abs(X - ref).max() < 1e-12 * np.abs(ref).max()


def test_inverse_passes_reproduce_irfft():
    rng = np.random.default_rng(1)
    Y = rng.standard_normal(201) + 1j * rng.standard_normal(201)
    x = inverse(Y)
    ref = np.fft.irfft(Y, N)                                   # numpy also ignores the imaginary parts of DC / Nyquist
    assert np.abs(x - ref).max() < 1e-12 * np.abs(ref).max()
    assert np.abs(inverse(np.fft.rfft(ref)) - ref).max() < 1e-12


def test_generated_tables_match_the_model():
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmgan_amd", "csrc", "stft_fft_tables.h")
    text = open(path).read()
    for name, want in (("fft_tw400", [W(400, r * k) for r in range(16) for k in range(13)]),
                       ("fft_tw25", [W(25, b * c) for b in range(5) for c in range(5)]),
                       ("fft_tw16", [W(16, q * s) for q in range(4) for s in range(4)])):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", text, re.S).group(1)
        vals = np.array([float(v.rstrip("f")) for v in re.findall(r"-?[\d.]+(?:e-?\d+)?f", body)]).reshape(-1, 2)
        got = vals[:, 0] + 1j * vals[:, 1]
        assert got.shape == (len(want),) and np.abs(got - np.array(want)).max() < 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# Index maps of the two kernels over whole clips (cmgan_amd/csrc/stft_fft.hip): which samples a forward wave stages for
# which frame, which rows it stores, and which frames the inverse's overlap-add sums into which output sample.  Modelled
# with the kernels' own expressions, checked against torch's reflect padding and torch.istft for every L in 201..3000.
# ---------------------------------------------------------------------------------------------------------------------
HOP = 100


def forward_group_load(L, t0):
    """Sample indices wave t0 / 4 stages in LDS (704 of them) - stft_fft400_kernel's interior / edge branch."""
    start = HOP * t0 - 200
    i = np.arange(704)
    if start >= 0 and start + 704 <= L:                       # interior group: plain loads
        return start + i
    sidx = start + i
    sidx = np.where(sidx < 0, -sidx, sidx)                    # reflect (torch.stft center=True)
    sidx = np.where(sidx >= L, 2 * (L - 1) - sidx, sidx)
    return np.clip(sidx, 0, L - 1)                            # frames past T in the last group


def forward_store(T, t0, lane_range=range(64)):
    """Offsets (relative to row t0 of one part) that the wave stores, each with the staging index it copies."""
    nfr = min(T - t0, 4)
    out = []
    for lane in lane_range:
        if nfr == 4:
            out += [lane + 64 * k for k in range(12)]
            if lane < 36:
                out.append(768 + lane)
        else:
            out += list(range(lane, nfr * 201, 64))
    return np.array(sorted(out))


def test_forward_group_loads_and_row_stores_cover_every_frame_like_torch_stft():
    """For every L in 201..3000: each stored frame t holds exactly padded[100 t : 100 t + 400] of torch's reflect pad,
    every load is inside the clip, and the waves store each of the T x 201 outputs of a part exactly once."""
    import torch
    import torch.nn.functional as Fn
    for L in range(201, 3001):
        T = L // HOP + 1
        padded = Fn.pad(torch.arange(L, dtype=torch.float64)[None, None], (200, 200), mode="reflect")[0, 0].long().numpy()
        written = np.zeros(T * 201, int)
        for t0 in range(0, 4 * ((T + 3) // 4), 4):             # every wave of the grid with t0 < T
            assert t0 < T
            src = forward_group_load(L, t0)
            assert src.min() >= 0 and src.max() < L, (L, t0)
            nfr = min(T - t0, 4)
            for j in range(nfr):                             # pass 1 lane (j, r) reads sg[100 j + 16 m + r]
                n = 16 * np.arange(25)[:, None] + np.arange(16)[None, :]
                got = src[HOP * j + n].reshape(-1)
                want = padded[HOP * (t0 + j) + n].reshape(-1)
                assert np.array_equal(got, want), (L, t0 + j)
            offs = forward_store(T, t0)
            assert np.array_equal(offs, np.arange(nfr * 201)), (L, t0)      # each staged value once, nothing beyond
            written[t0 * 201 + offs] += 1
        assert (written == 1).all(), L


def inverse_block_frames(T, blk):
    """{slot fs: frame t} that the five waves of istft_fft400_kernel block blk transform ([ja, jb) and the wv == 4 cut),
    and the rows pass A reads (clamped into [ja, jb))."""
    slots, rows = {}, set()
    for wv in range(5):
        tw0 = 16 * blk - 1 + 4 * wv
        ja = -tw0 if tw0 < 0 else 0
        jb = (0 if T - tw0 < 0 else T - tw0) if T - tw0 < 4 else 4
        if wv == 4 and jb > 3:
            jb = 3
        if jb > ja:
            for jr in range(4):                              # pass A's clamped row of every (frame, channel) lane
                rows.add(tw0 + (ja if jr < ja else (jb - 1 if jr >= jb else jr)))
            for j in range(ja, jb):                          # pass B: lane (j, r) for j in [ja, jb)
                slots[4 * wv + j] = tw0 + j
    return slots, rows


def inverse_ola_terms(T, blk, Lout):
    """{output sample s: [(frame t, slot fs, sample n)]} of the block's overlap-add (kept samples only), plus the slots
    read by any thread with ok set (stored or not)."""
    terms, used = {}, set()
    for tid in range(320):
        for i in range(5):
            sl = tid + 320 * i
            s = 1600 * blk + sl
            fs0, n0 = sl // HOP, 300 + sl % HOP
            acc = []
            for q in range(4):
                fs, n = fs0 + q, n0 - HOP * q
                t = 16 * blk - 1 + fs
                if 0 <= t < T:
                    acc.append((t, fs, n))
                    used.add(fs)
            if s < Lout:
                terms[s] = acc
    return terms, used


def test_inverse_block_frames_and_overlap_add_sum_what_torch_istft_sums():
    """For every output length 100 (T - 1) up to 6400 (T = 2 .. 65: 1 .. 4 blocks, every position of the last frame in
    its block): pass A reads only rows inside [0, T); every frame a sample needs is transformed in the slot the OLA reads;
    each output sample sums exactly the frames whose 400-sample support covers it in torch.istft's centred frame grid,
    each once; every transformed frame is used; and the OLA of random frames through these maps equals torch.istft."""
    import torch
    win = torch.hamming_window(400, dtype=torch.float64)
    rng = np.random.default_rng(7)
    for T in range(2, 66):
        Lout = HOP * (T - 1)
        nblk = (Lout + 1599) // 1600
        frames = rng.standard_normal((T, 400))                 # un-windowed frames g[t]
        out = np.full(Lout, np.nan)
        w = win.numpy()
        for blk in range(nblk):
            slots, rows = inverse_block_frames(T, blk)
            assert all(0 <= r < T for r in rows), (T, blk)
            terms, used = inverse_ola_terms(T, blk, Lout)
            assert set(slots) == used, (T, blk)                # nothing transformed for nothing, nothing read unwritten
            assert max(slots) <= 18
            for s, acc in terms.items():
                p = s + 200                                  # centre trim
                want = sorted(t for t in range(T) if 0 <= p - HOP * t < 400)
                assert sorted(t for t, _, _ in acc) == want, (T, s)
                for t, fs, n in acc:
                    assert slots[fs] == t and n == p - HOP * t
                acc_v = sum(frames[t, n] * w[n] for t, _, n in acc)
                env = sum(w[n] * w[n] for _, _, n in acc)
                assert np.isnan(out[s])
                out[s] = acc_v / env
        assert not np.isnan(out).any(), T
        spec = torch.fft.rfft(torch.from_numpy(frames), dim=-1).T          # [F, T]: irfft(spec[:, t]) == g[t]
        ref = torch.istft(spec, 400, HOP, window=win, center=True).numpy()
        assert ref.shape == (Lout,)
        assert np.abs(out - ref).max() < 1e-12 * np.abs(ref).max(), T
