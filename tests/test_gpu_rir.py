"""The room simulator on the GPU (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses"): Engine.rir
against the float64 numpy model of tests/rir_model.py over the kernel's tile and list edges, truncated and oversized
image ranges, invalid rows, bit-reproducibility and row independence, hipGraph replay with the room table changed in
place, and the front end (RirBank.simulate, DynamicMixer(rooms=...), MixingLoader) through Engine.mix against the two
models chained.

The bound, for every tap (rir_model.bound):    |gpu[k] - h[k]| <= 2^-24 |h[k]| + 64 * 2^-53 * (K + tw) * A[k]
with A[k] = sum |a| over the images whose window reaches tap k.  2^-24 |h| is the one rounding to float32.  The second
term allows some 40 ulps of error in tau - an ulp of tau is at most 2^-53 (K + tw) samples and |d sinc / dt| < pi / 2 - plus
the amplitude's few ulps.  The kernel's two shortcuts stay inside it: the Hann term by angle addition,
cos(pi (j + t0) / tw) from cos / sin of pi j / tw and of pi t0 / tw, is four correctly rounded factors and three
operations, an absolute error of a few 2^-53 on a quantity <= 1, against an allowance of 64 (K + tw) >= 16000 of them
at the smallest K here; and t = j + (k0 - tau) instead of k - tau is one more rounding of at most an ulp of K."""
import numpy as np
import pytest
import torch

import mix_model as MM
import rir_cases as RC
import rir_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, C = 16000, 343.0
U32, U64 = 2.0 ** -24, 2.0 ** -53

ROOM = [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]      # the reciprocity room
N5 = (5, 5, 5)                 # every image a response of up to 700 + 40 samples can see in ROOM


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def TILE():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_rir_tile())


def _run(eng, rooms, n_taps, K, N, tw=40, out=None):
    rooms_d = torch.tensor(np.asarray(rooms, dtype=np.float64).reshape(-1, 15), device=DEV)
    taps_d = torch.tensor(np.asarray(n_taps, dtype=np.int32).reshape(-1), device=DEV)
    rir, length = eng.rir(rooms_d, taps_d, K, N, fs=FS, c=C, tw=tw, out=out)
    assert rir.dtype == torch.float32 and tuple(rir.shape) == (rooms_d.size(0), K) and length.dtype == torch.int32
    return rir.cpu().numpy(), length.cpu().numpy()


def _check(tag, got, rooms, n_taps, K, N, tw=40, model_N=None):
    """Every row of `got` against the model under the bound; taps >= k_r bit-zero; lengths.  Returns the worst ratio."""
    rir, length = got
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    worst = 0.0
    for r in range(rooms.shape[0]):
        h, A, kr = M.rir_row(rooms[r], int(np.asarray(n_taps).reshape(-1)[r]), K, model_N or N, FS, C, tw)
        assert length[r] == kr, f"{tag} row {r}: len {length[r]}, model {kr}"
        assert not rir[r, kr:].view(np.uint32).any(), f"{tag} row {r}: taps >= k_r are not bit-zero"
        err, bd = np.abs(rir[r].astype(np.float64) - h), M.bound(h, A, K, tw)
        bad = err > bd
        assert not bad.any(), (f"{tag} row {r}: {int(bad.sum())} of {K} taps outside the bound, first at {int(np.argmax(bad))}, "
                               f"worst err {err[bad].max():.3e} at bound {bd[bad][np.argmax(err[bad])]:.3e}")
        if kr > 1 and M.row_is_valid(rooms[r]):
            assert np.max(np.abs(h)) > 0.0
        worst = max(worst, float(np.max(err[bd > 0] / bd[bd > 0])) if (bd > 0).any() else 0.0)
    return worst


# ------------------------------------------------------------------ 1. the kernels against the model
@pytest.mark.parametrize("tw", [4, 40])
@pytest.mark.parametrize("k_of_tile", [lambda T: T - 1, lambda T: T, lambda T: T + 1, lambda T: 2 * T + 3, lambda T: 700],
                         ids=["TILE-1", "TILE", "TILE+1", "2TILE+3", "700"])
def test_kernel_matches_the_float64_model(eng, TILE, k_of_tile, tw):
    K = k_of_tile(TILE)
    got = _run(eng, ROOM, [K], K, N5, tw)
    worst = _check(f"K={K} tw={tw}", got, ROOM, [K], K, N5, tw)
    print(f"[rir] K={K} tw={tw}: worst error / bound {worst:.3f}")


def test_three_different_rooms_in_one_call(eng, TILE):
    K = 2 * TILE + 3
    dead = [4.0, 5.0, 3.0, 0.5, 1.0, 1.0, 3.2, 1.7, 1.4] + [0.0] * 6                      # every wall absorbs everything
    one_zero = [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.0, 0.8, 0.85, 0.75, 0.9]   # one absorbing wall
    rooms, n_taps, N = [ROOM, dead, one_zero], [K, K - 17, 1], (4, 5, 4)
    got = _run(eng, rooms, n_taps, K, N)
    _check("three rooms", got, rooms, n_taps, K, N)
    assert got[1].tolist() == [K, K - 17, 1]
    assert np.count_nonzero(got[0][1]) == 2 * 40 and np.count_nonzero(got[0][0]) > K // 2     # (dead: the direct path's window)


@pytest.mark.parametrize("name,room", [
    # a source 5 cm from the wall at x = 0: each image pair (p_x = 0, 1) is 10 cm apart, 4.7 samples
    ("source at a wall", [3.0, 4.0, 2.5, 0.05, 2.0, 1.2, 2.5, 1.0, 1.0, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
    # a direct path of 0.245 m = 11.4 samples, shorter than tw = 40: its window is cut at k < 0
    ("direct path inside the window", [3.0, 4.0, 2.5, 1.0, 1.0, 1.0, 1.2, 1.1, 0.9, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
    # source on the receiver: d = 0 is held at CMGAN_RIR_DMIN in the amplitude
    ("source on the receiver", [3.0, 4.0, 2.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
])
def test_close_images_and_windows_cut_at_zero(eng, TILE, name, room):
    K, N = TILE + 44, (3, 2, 3)
    got = _run(eng, room, [K], K, N)
    _check(name, got, room, [K], K, N)


def test_image_range_smaller_and_larger_than_the_response_needs(eng):
    K = 700
    full = _run(eng, ROOM, [K], K, N5)
    # N = 1 cuts images that the time range would admit: the result is the model's with the same N, and another response
    cut = _run(eng, ROOM, [K], K, (1, 1, 1))
    _check("N=(1,1,1)", cut, ROOM, [K], K, (1, 1, 1))
    assert not np.array_equal(cut[0], full[0])
    for N in [(0, 0, 0), (2, 0, 1)]:
        _check(f"N={N}", _run(eng, ROOM, [K], K, N), ROOM, [K], K, N)
    # N larger than needed: the extra images add nothing - the model's result with the large N, the bits of the small one
    big = _run(eng, ROOM, [K], K, (9, 8, 10))
    _check("N=(9,8,10)", big, ROOM, [K], K, (9, 8, 10))
    assert np.array_equal(big[0].view(np.uint32), full[0].view(np.uint32))
    huge = _run(eng, ROOM, [K], K, (40, 3, 70))                   # (Ny = 3 cuts; compare with the same cut)
    small = _run(eng, ROOM, [K], K, (5, 3, 5))
    assert np.array_equal(huge[0].view(np.uint32), small[0].view(np.uint32))


def test_more_images_in_a_tile_than_the_on_chip_list_holds(eng, TILE):
    """A small, lively room: the images that reach the last tile are more than twice cmgan_rir_list_capacity(), so a
    round of the scan overflows the list and is consumed in chunks."""
    from cmgan_amd import _lib
    cap = int(_lib.load().cmgan_rir_list_capacity())
    room = [1.2, 1.2, 1.2, 0.3, 0.4, 0.5, 0.9, 0.8, 0.7] + [0.97] * 6
    K, N = 3 * TILE, (9, 9, 9)                                    # ceil((K + 40) c / fs / 2.4) + 1 = 9
    tau = M.images(room, N)[0] * FS / C
    reach = (tau > K - TILE - 40) & (tau < K - 1 + 40)
    in_last = int(np.sum(reach))
    assert in_last > 2 * cap, (in_last, cap)
    # the scan takes the columns (nx, ny, p) - rir_model.images' order with nz innermost - in rounds of one per thread
    per_col = reach.reshape(-1, 2 * N[2] + 1).sum(1)
    per_round = np.add.reduceat(per_col, np.arange(0, per_col.size, TILE))
    assert per_round.max() > cap, (per_round.max(), cap)
    got = _run(eng, room, [K], K, N)
    worst = _check("lively cube", got, room, [K], K, N)
    print(f"[rir] {in_last} images in the last tile (capacity {cap}): worst error / bound {worst:.3f}")


# ------------------------------------------------------------------ 2. the contract
def test_invalid_rows_are_zeros_with_length_one(eng, TILE):
    K, N = TILE + 9, (2, 2, 2)
    other = [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.7, 0.8, 0.85, 0.75, 0.9]
    bad = []
    for at, v in [(4, np.nan), (1, -2.0), (12, 1.5), (0, 0.0), (7, np.inf), (9, -1e-9)]:
        row = list(ROOM)
        row[at] = v
        bad.append(row)
    rooms = [ROOM, bad[0], bad[1], other, bad[2], bad[3], bad[4], bad[5], ROOM]
    n_taps = [K] * len(rooms)
    out = (torch.full((len(rooms), K), 7.0, dtype=torch.float32, device=DEV),
           torch.full((len(rooms),), -5, dtype=torch.int32, device=DEV))
    rir, length = _run(eng, rooms, n_taps, K, N, out=out)
    assert length.tolist() == [K, 1, 1, K, 1, 1, 1, 1, K]
    for r in (1, 2, 4, 5, 6, 7):
        assert not rir[r].view(np.uint32).any(), r
    _check("invalid rows", (rir, length), rooms, n_taps, K, N)
    for r, room in ((0, ROOM), (3, other), (8, ROOM)):            # the neighbours are what they are alone
        alone = _run(eng, room, [K], K, N)
        assert np.array_equal(alone[0][0].view(np.uint32), rir[r].view(np.uint32)), r


def test_bit_identical_between_calls_and_row_independent(eng, TILE):
    K, N = 2 * TILE + 50, (4, 4, 4)
    rooms = [ROOM,
             [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.7, 0.8, 0.85, 0.75, 0.9],
             [1.5, 1.7, 1.4, 0.4, 0.5, 0.6, 1.1, 1.2, 0.9, 0.95, 0.9, 0.92, 0.97, 0.9, 0.93]]
    n_taps = [K, TILE + 1, K - 3]
    a = _run(eng, rooms, n_taps, K, N)
    b = _run(eng, rooms, n_taps, K, N)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    for r in range(3):
        one = _run(eng, rooms[r], n_taps[r:r + 1], K, N)
        assert np.array_equal(one[0][0].view(np.uint32), a[0][r].view(np.uint32)), r
        assert one[1][0] == a[1][r]


def test_captured_call_replays_with_a_new_room_table(eng, TILE):
    K, N = TILE + 30, (3, 3, 3)
    rooms = torch.tensor([ROOM, ROOM], dtype=torch.float64, device=DEV)
    n_taps = torch.tensor([K, K], dtype=torch.int32, device=DEV)
    eager, eager_len = eng.rir(rooms, n_taps, K, N)               # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_rir, g_len = eng.rir(rooms, n_taps, K, N)
    graph.replay()
    assert torch.equal(g_rir, eager) and torch.equal(g_len, eager_len)
    # a new table and new lengths, written in place into the tensors the graph reads
    new = torch.tensor([[3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.7, 0.8, 0.85, 0.75, 0.9],
                        [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.5, 0.8, float("nan"), 0.7, 0.6, 0.95]],
                       dtype=torch.float64, device=DEV)
    rooms.copy_(new)
    n_taps.copy_(torch.tensor([K - 40, K], dtype=torch.int32, device=DEV))
    graph.replay()
    again, again_len = eng.rir(rooms, n_taps, K, N)
    assert not torch.equal(again, eager)
    assert torch.equal(g_rir, again) and torch.equal(g_len, again_len)
    assert again_len.tolist() == [K - 40, 1]
    _check("replayed", (g_rir.cpu().numpy(), g_len.cpu().numpy()), new.cpu().numpy(), [K - 40, K], K, N)


# ------------------------------------------------------------------ 3. the front end
def _small_sampler(seed):
    from cmgan_amd.mixing import RoomSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return RoomSampler(dims=((2.0, 2.0, 2.0), (3.0, 3.0, 2.5)), rt60=(0.06, 0.2), margin=0.3, generator=gen)


def _model_bank(rooms, n_taps, K, N, rows):
    """The model's responses as the float32 bank Engine.mix would be given, `rows` rows (an identity row appended if
    rows > len(rooms)), with per tap dh >= |gpu float32 - model float32|: both round a value within the kernel's bound
    of h, so they differ by at most the bound plus the model's own rounding."""
    h, A, length = M.rir(rooms, n_taps, K, N, FS, C, 40)
    bank = np.zeros((rows, K), dtype=np.float32)
    bank[:len(h)] = h.astype(np.float32)
    dh = np.zeros((rows, K))
    dh[:len(h)] = M.bound(h, A, K, 40) + U32 * np.abs(h)
    if rows > len(h):
        bank[len(h), 0] = 1.0
    return bank, dh, length


def _check_mix(tag, noisy, target, rows, clean, bank, dh, idx, rlen, L, early):
    """Engine.mix on the GPU's responses against mix_model on the model's responses, peak guard off (scale == 1).  The
    responses differ by dh per tap, so speech and the early target by at most E = max|clean| sum_k dh[k]; Ps = mean
    speech^2 then moves by at most 2 E sqrt(Ps) (Cauchy-Schwarz), g = sqrt(Ps / (Pn c)) by g E / sqrt(Ps), and that reaches
    noisy through g |n|.  To these first-order terms (given 1 % for the second order) come the rounding to float32 and the
    summation-order terms of test_gpu_mix."""
    for b, r in enumerate(rows):
        assert r["scale"] == 1.0
        k = int(rlen[b])
        h = bank[int(idx[b]), :k].astype(np.float64)
        xmax = float(np.max(np.abs(clean[b])))
        E = 1.01 * xmax * float(np.sum(dh[int(idx[b]), :k])) + 2.0 * k * U64 * float(np.sum(np.abs(h))) * xmax
        dg = r["g"] * E / np.sqrt(r["Ps"]) * 1.01 + 2.0 * L * U64 * r["g"]
        bound_n = U32 * np.abs(r["noisy"]) + E + dg * np.abs(r["noise"])
        bound_t = U32 * np.abs(r["target"]) + (E if early >= 0 else 0.0)
        for name, a, w, bd in (("noisy", noisy[b], r["noisy"], bound_n), ("target", target[b], r["target"], bound_t)):
            err = np.abs(a.astype(np.float64) - w)
            bad = err > bd
            assert not bad.any(), (f"{tag} row {b} {name}: {int(bad.sum())} of {L} outside the bound, worst "
                                   f"err {err[bad].max():.3e} at bound {bd[bad][np.argmax(err[bad])]:.3e}")
            assert np.max(np.abs(w)) > 0.0


def test_simulated_bank_feeds_the_mixer(eng):
    from cmgan_amd.mixing import RirBank
    sampler = _small_sampler(21)
    R, seconds = 3, 0.1
    bank = RirBank.simulate(eng, sampler, R, seconds=seconds, sample_rate=FS)
    K, N = 1600, sampler.n_images(1600, FS)
    assert tuple(bank.data.shape) == (R, K) and bank.length.dtype == torch.int32 and tuple(bank.rooms.shape) == (R, 15)
    rooms, length = bank.rooms.cpu().numpy(), bank.length.cpu().numpy()
    assert np.all(length >= int(0.06 * FS)) and np.all(length <= K)
    _check("simulate", (bank.data.cpu().numpy(), length), rooms, length, K, N)
    rng = np.random.default_rng(22)
    B, L, early = 4, 2100, 160
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    noise = rng.standard_normal(3000).astype(np.float32)
    start, nlen = np.array([0, 100, 500, 0], dtype=np.int64), np.array([3000, 700, 2500, 1], dtype=np.int64)
    off = np.array([5, 9999, 0, 0], dtype=np.int64)
    snr = np.array([0.0, 5.0, 10.0, 20.0], dtype=np.float32)
    idx = np.array([0, 1, 2, 1], dtype=np.int32)
    rlen = length[idx].astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    noisy, target, info = eng.mix(t(clean), t(noise), t(start), t(nlen), t(off), t(snr), bank.data, t(idx), t(rlen),
                                  peak=100.0, early=early)
    mbank, dh, mlen = _model_bank(rooms, length, K, N, R)
    assert np.array_equal(mlen, length)
    rows = MM.mix_batch(clean, noise, start, nlen, off, snr, mbank, idx, rlen, 100.0, early)
    _check_mix("simulated bank", noisy.cpu().numpy(), target.cpu().numpy(), rows, clean, mbank, dh, idx, rlen, L, early)


def test_dynamic_mixer_with_a_room_per_row(eng):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(23)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (1, 300, 5000)], device=DEV)
    B, L = 8, 2100
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    cd = torch.from_numpy(clean).to(DEV)

    def mixer(seed):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        return DynamicMixer(eng, nb, rooms=_small_sampler(seed + 100), snr_db=(0.0, 15.0), early_ms=10.0, p_reverb=0.5,
                            peak=100.0, generator=gen, rir_seconds=0.1)

    m1, m2 = mixer(5), mixer(5)
    K = m1.rir_taps
    assert K == 1600 and m1.early == 160 and m1.n_images == m1.rooms.n_images(K, FS)
    t1, n1, i1 = m1(cd)
    t2, n2, i2 = m2(cd)
    assert torch.equal(t1, t2) and torch.equal(n1, n2) and all(torch.equal(a, b) for a, b in zip(i1, i2))
    d = m1.last_draw
    idx, rlen, rooms = d.rir_index.cpu().numpy(), d.rir_len.cpu().numpy(), d.rooms.cpu().numpy()
    wet = idx != B
    assert tuple(rooms.shape) == (B, 15) and np.array_equal(idx[wet], np.arange(B)[wet]) and np.all(rlen[~wet] == 1)
    sim = m1.last_bank
    assert tuple(sim.data.shape) == (B + 1, K) and sim.data[B].cpu().tolist() == [1.0] + [0.0] * (K - 1)
    assert np.array_equal(sim.length.cpu().numpy()[:B], rlen) and int(sim.length[B]) == 1
    mbank, dh, _ = _model_bank(rooms, rlen, K, m1.n_images, B + 1)
    g = lambda v: v.cpu().numpy()
    rows = MM.mix_batch(clean, g(nb.data), g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db), mbank, idx, rlen,
                        100.0, m1.early)
    _check_mix("rooms mixer", n1.cpu().numpy(), t1.cpu().numpy(), rows, clean, mbank, dh, idx, rlen, L, m1.early)
    for b in np.flatnonzero(~wet):                                # a dry row: the target is the clip itself
        assert torch.equal(t1[b], cd[b])
    # the next call draws other rooms into the SAME allocation
    ptr = sim.data.data_ptr()
    t1b, n1b, _ = m1(cd)
    t2b, n2b, _ = m2(cd)
    assert torch.equal(n1b, n2b) and not torch.equal(n1b, n1)
    assert m1.last_bank.data.data_ptr() == ptr and not torch.equal(m1.last_draw.rooms, d.rooms)


def test_mixing_loader_with_rooms_feeds_a_generator_train_step(eng):
    from cmgan_amd.mixing import DynamicMixer, MixingLoader, NoiseBank
    from cmgan_amd.training import AdamW, GeneratorTrain, generator_train_step
    from oracle.weights import make_state_dict
    rng = np.random.default_rng(24)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (300, 5000)], device=DEV)
    B, L = 2, 3200
    clips = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    loader = torch.utils.data.DataLoader([(torch.from_numpy(clips[i]), L) for i in range(B)], batch_size=B, shuffle=False)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    mixer = DynamicMixer(eng, nb, rooms=_small_sampler(31), snr_db=(0.0, 20.0), early_ms=10.0, generator=gen, rir_seconds=0.1)
    target, noisy, length = next(iter(MixingLoader(loader, mixer)))
    assert target.is_cuda and noisy.is_cuda and tuple(noisy.shape) == (B, L) and length.tolist() == [L] * B
    assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(target).all())
    assert float(target.abs().max()) > 0.0 and not torch.equal(target.cpu(), torch.from_numpy(clips))    # reverberant
    net = GeneratorTrain(make_state_dict(seed=0), engine=eng)
    opt = AdamW(eng, net.param_bucket, net.grad_bucket, lr=5e-4)
    loss, terms = generator_train_step(net, opt, target, noisy)
    assert np.isfinite(float(loss)) and bool(torch.isfinite(terms).all())


# ------------------------------------------------------------------ 4. the recorded bits
@pytest.mark.parametrize("name", RC.RIR_NAMES)
def test_the_bits_are_the_recorded_ones(eng, TILE, name):
    """Engine.rir on the cases of tests/rir_cases.py against tests/golden/rir_parent_bits.npz (make_rir_bits.py): the
    model-based tests above bound the error, this one sees a changed rounding or a changed enumeration order."""
    import os
    from mixer_cases import assert_recorded_bits
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rir_parent_bits.npz"))
    assert_recorded_bits(f"rir/{name}", RC.run(eng, RC.rir_cases(TILE)[name], DEV), want)
