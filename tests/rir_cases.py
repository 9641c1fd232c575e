"""The room-simulator cases whose output bits are recorded at one commit and replayed at every later one
(tests/golden/make_rir_bits.py; tests/test_gpu_rir.py, tests/test_gpu_rir_bands.py), as literal tables and seeds keyed by
T = cmgan_rir_tile(): one definition of every case, so the recorder and its tests cannot drift apart.  Each case is the
smallest shape at which one piece of the image enumeration that cmgan_rir and cmgan_rir_bands share can go wrong: the
tile edges, a short and a long window, image ranges larger than needed, rows of different lengths beside an invalid
one, and a round of the scan that overflows the on-chip list.  `nontrivial` states what keeps a case from passing
empty-handed; the recorder asserts it of the GPU's output, the host tests of the float64 models'."""
import numpy as np
import torch

import rir_model as M

FS, C = 16000, 343.0
GEOMETRY = [4.0, 3.0, 2.5, 1.1, 0.9, 1.3, 2.9, 2.2, 1.6]                                   # size, source, receiver
WALLS = [0.9, 0.8, 0.85, 0.7, 0.6, 0.95]
ROOM = GEOMETRY + WALLS                                                                    # the 4 x 3 x 2.5 m room
NEVER_READ = [float("nan")] * 6                                                            # columns 9 - 14 of a banded row
CUBE = [1.2, 1.2, 1.2, 0.3, 0.4, 0.5, 0.9, 0.8, 0.7]                                       # the lively 1.2 m cube
# the three rooms of test_gpu_rir.py::test_three_different_rooms_in_one_call, and the first of them with a NaN
SMALL = [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]
DEAD = [4.0, 5.0, 3.0, 0.5, 1.0, 1.0, 3.2, 1.7, 1.4] + [0.0] * 6
ONE_ZERO = [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.0, 0.8, 0.85, 0.75, 0.9]
INVALID = SMALL[0:4] + [float("nan")] + SMALL[5:]


def images_for(taps, tw, size):
    """The image ranges that leave out no image of a response of `taps` taps."""
    reach = (taps + tw) * C / FS
    return tuple(int(np.ceil(reach / (2 * l))) + 1 for l in size)


def band_table(NB, walls=WALLS, air=0.004):
    """Band b: the walls a little more absorbing per band, m_b = air b."""
    return np.array([[w * (1.0 - 0.05 * b) for w in walls] + [air * b] for b in range(NB)])


def filters(NB, NF):
    """A seeded filterbank [NB, NF]: a delta of weight 1 - b / 8 at the centre plus noise of unit energy in all."""
    g = np.random.default_rng(1000 * NB + NF).standard_normal((NB, NF)) / np.sqrt(NB * NF)
    g[:, (NF - 1) // 2] += 1.0 - 0.125 * np.arange(NB)
    return g


def rir_cases(T):
    """name -> dict(rooms [R][15], n_taps [R], K, N, tw, live rows) of Engine.rir."""
    K = 2 * T + 3
    need = images_for(K, 40, ROOM[0:3])
    one = lambda room, K, N, tw: dict(rooms=[room], n_taps=[K], K=K, N=N, tw=tw, live=[0])
    return {
        "room/tw4": one(ROOM, K, images_for(K, 4, ROOM[0:3]), 4),
        "room/tw40": one(ROOM, K, need, 40),
        "room/larger-ranges": one(ROOM, K, (need[0] + 4, need[1] + 9, need[2] + 30), 40),
        "three-rooms": dict(rooms=[SMALL, DEAD, ONE_ZERO, INVALID], n_taps=[K, K - 17, 1, K], K=K, N=(4, 5, 4), tw=40, live=[0],
                            invalid=[3]),
        "cube": one(CUBE + [0.97] * 6, 3 * T, (9, 9, 9), 40),
    }


def rir_bands_cases(T):
    """name -> dict(rooms [R][15], bands [R][NB][7], n_taps [R], K, filt [NB][NF], N, tw, live rows) of Engine.rir_bands."""
    K = 2 * T + 3
    banded = GEOMETRY + NEVER_READ

    def one(room, bands, K, NF, tw, size=ROOM[0:3]):
        return dict(rooms=[room], bands=[bands], n_taps=[K], K=K, filt=filters(len(bands), NF),
                    N=images_for(K + (NF - 1) // 2, tw, size), tw=tw, live=[0])

    dead = np.zeros((3, 7))                                       # every wall absorbs everything in every band
    dead[:, 6] = [0.0, 0.01, 0.02]
    one_zero = band_table(3, [w * z for w, z in zip(WALLS, (1, 0, 1, 1, 1, 1))], air=0.0)      # one absorbing wall, m = 0
    broken = band_table(3)
    broken[1, 2] = np.nan
    cube_bands = np.array([[0.97 - 0.01 * b] * 6 + [0.002 * b] for b in range(3)])
    return {
        "room/nb1-nf1": one(banded, band_table(1), K, 1, 40),
        "room/nb3-nf9": one(banded, band_table(3), K, 9, 40),
        "room/nb8-nf1023": one(banded, band_table(8), K, 1023, 40),
        "room/tile-edge": one(banded, band_table(3), T - 1, 9, 4),                            # K + D = T + 3
        "cube": one(CUBE + [0.0] * 6, cube_bands, 3 * T - 4, 9, 40, CUBE[0:3]),               # K + D = 3 T
        "three-rooms": dict(rooms=[banded, [4.0, 3.0, 2.5, 0.5, 1.0, 1.0, 3.2, 1.7, 1.4] + [0.3] * 6,
                                   [4.0, 3.0, 2.5, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8] + [0.0] * 6, banded],
                            bands=[band_table(3), dead, one_zero, broken], n_taps=[K, K - 17, 1, K], K=K, filt=filters(3, 9),
                            N=images_for(K + 4, 40, ROOM[0:3]), tw=40, live=[0], invalid=[3]),
    }


def images_in_the_last_tile(case, T):
    """How many images of row 0 reach the last tile of the tap kernel (K + D taps for a banded case)."""
    room = np.array(case["rooms"][0], dtype=np.float64)
    taps = case["K"]
    if "bands" in case:
        room[9:15] = np.asarray(case["bands"][0])[0, 0:6]
        taps += (np.asarray(case["filt"]).shape[1] - 1) // 2
    tau = M.images(room, case["N"])[0] * FS / C
    k0 = (taps - 1) // T * T
    return int(np.sum((tau > k0 - case["tw"]) & (tau < taps - 1 + case["tw"])))


def nontrivial(name, case, rir, length, T, cap):
    """A case does not pass empty-handed: a peak above 0.01, more than K / 2 non-zero taps in every live row, and in the
    cube more than 2 `cap` (cmgan_rir_list_capacity()) images in the last tile."""
    rir, K = np.asarray(rir), case["K"]
    assert np.asarray(length).tolist() == [1 if r in case.get("invalid", ()) else min(max(n, 1), K)
                                          for r, n in enumerate(case["n_taps"])], name
    assert float(np.max(np.abs(rir))) > 0.01, (name, float(np.max(np.abs(rir))))
    for r in case["live"]:
        assert np.count_nonzero(rir[r]) > K // 2, (name, r, int(np.count_nonzero(rir[r])), K)
    if name == "cube":
        assert images_in_the_last_tile(case, T) > 2 * cap, (name, images_in_the_last_tile(case, T), cap)


def run(eng, case, device):
    """The case through Engine.rir or Engine.rir_bands: {"rir": float32 [R, K], "len": int32 [R]} on the device."""
    t = lambda a, dt: torch.tensor(np.asarray(a, dtype=dt), device=device)
    rooms, n_taps = t(case["rooms"], np.float64), t(case["n_taps"], np.int32)
    if "bands" in case:
        rir, length = eng.rir_bands(rooms, t(case["bands"], np.float64), n_taps, case["K"], t(case["filt"], np.float64),
                                    case["N"], fs=FS, c=C, tw=case["tw"])
    else:
        rir, length = eng.rir(rooms, n_taps, case["K"], case["N"], fs=FS, c=C, tw=case["tw"])
    return {"rir": rir, "len": length}


def model(case):
    """The case through the float64 models: (h float64 [R, K], len int32 [R])."""
    if "bands" in case:
        import rir_bands_model as BM
        h, _, length = BM.rir_bands(case["rooms"], case["bands"], case["n_taps"], case["K"], case["N"], case["filt"], FS, C,
                                    case["tw"])
    else:
        h, _, length = M.rir(case["rooms"], case["n_taps"], case["K"], case["N"], FS, C, case["tw"])
    return h, length


RIR_NAMES, RIR_BANDS_NAMES = tuple(rir_cases(1)), tuple(rir_bands_cases(1))            # (the names do not depend on T)
