"""CPU side of dynamic mixing (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Dynamic mixing"): the float64 model the GPU
tests compare the kernels with (tests/mix_model.py) against scipy and against its own definition, the workspace formula,
and every argument error of cmgan_mix and Engine.mix, all of which are judged before a handle or a GPU is needed."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import signal as sig

import mix_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import MIX_MAX_TAPS, check_mix_args

BADARG, UNSUPPORTED = -1, -3


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("L,K", [(1, 1), (2, 5), (257, 63), (1000, 1000), (300, 2000), (4000, 65)])
def test_model_convolution_matches_fftconvolve(L, K):
    rng = np.random.default_rng(L * 7 + K)
    x = rng.standard_normal(L).astype(np.float32)
    h = (rng.standard_normal(K) * np.exp(-np.arange(K) / (0.2 * K + 1))).astype(np.float32)
    d = M.direct_path(h)
    got = M.reverb(x, h, d)
    full = sig.fftconvolve(x.astype(np.float64), h.astype(np.float64))
    want = np.zeros(L)
    n = min(L, full.size - d)
    want[:n] = full[d:d + n]
    assert got.dtype == np.float64 and got.shape == (L,)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_model_convolution_is_the_defining_sum():
    rng = np.random.default_rng(3)
    x, h = rng.standard_normal(37), rng.standard_normal(11)
    for d in (0, 4, 10):
        for last in (d, d + 2, 10):
            want = np.array([sum(h[k] * x[i + d - k] for k in range(min(last, 10) + 1) if 0 <= i + d - k < 37)
                             for i in range(37)])
            assert np.allclose(M.reverb(x, h, d, last_tap=min(last, 10)), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_direct_path_index(where):
    K = 9
    at = {"first": 0, "middle": 4, "last": K - 1}[where]
    h = np.full(K, 0.25, dtype=np.float32)
    h[at] = -0.9                                                  # the largest MAGNITUDE, whatever its sign
    assert M.direct_path(h) == at
    x = np.arange(1, 21, dtype=np.float32)
    one = np.zeros(K, dtype=np.float32)
    one[at] = 1.0                                                 # a pure delay is removed: speech == clean
    assert np.array_equal(M.reverb(x, one, M.direct_path(one)), x.astype(np.float64))
    tie = np.zeros(K, dtype=np.float32)
    tie[[2, 6]] = [0.5, -0.5]
    assert M.direct_path(tie) == 2                                # the FIRST of equals


@pytest.mark.parametrize("length", [1, 7, 50])
def test_noise_wrap_rule(length):
    L, start, off = 20, 3, 5
    bank = np.arange(100, dtype=np.float32)
    n = M.wrap_noise(bank, start, length, off, L)
    assert n.shape == (L,)
    for i in range(L):
        assert n[i] == bank[start + (off + i) % length]
    assert n.min() >= start and n.max() < start + length          # never leaves the item
    if length == 1:
        assert np.all(n == bank[start])
    if length > L:
        assert np.array_equal(n, bank[start + off:start + off + L])


def test_gain_is_zero_for_silence_and_sets_the_snr():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(400).astype(np.float32) * 0.1
    bank = rng.standard_normal(300).astype(np.float32)
    r = M.mix_row(np.zeros(400, np.float32), bank, 0, 300, 0, 5.0)
    assert r["g"] == 0.0 and r["Ps"] == 0.0 and np.all(r["noisy"] == 0.0)
    r = M.mix_row(x, np.zeros(300, np.float32), 0, 300, 0, 5.0)
    assert r["g"] == 0.0 and r["Pn"] == 0.0 and np.array_equal(r["noisy"], x.astype(np.float64))
    r = M.mix_row(x, bank, 10, 200, 77, 5.0, peak=100.0)
    assert abs(10 * np.log10(r["Ps"] / (r["g"] ** 2 * r["Pn"])) - 5.0) < 1e-9


def test_peak_guard_on_and_off():
    rng = np.random.default_rng(6)
    x = rng.standard_normal(500).astype(np.float32) * 0.05
    bank = rng.standard_normal(500).astype(np.float32)
    h = np.array([0.2, 1.0, 0.5, 0.25], dtype=np.float32)
    off = M.mix_row(x, bank, 0, 500, 0, 20.0, h, peak=0.99, early=-1)
    assert off["scale"] == 1.0 and np.array_equal(off["target"], x.astype(np.float64))
    on = M.mix_row(x, bank, 0, 500, 0, -30.0, h, peak=0.99, early=1)
    pk = float(np.float32(0.99))
    assert on["scale"] < 1.0 and abs(np.max(np.abs(on["noisy"])) - pk) <= 1e-15
    want_t = M.reverb(x, h, 1, last_tap=2) * on["scale"]          # the target carries the same scale
    assert np.array_equal(on["target"], want_t)


# ------------------------------------------------------------------ workspace
def test_workspace_bytes_monotone_and_rejects_unsupported_shapes():
    lib = _lib.load()
    ws = lambda B, L, K: int(lib.cmgan_mix_workspace_bytes(None, B, L, K))
    tile = lib.cmgan_mix_tile()
    assert tile > 0 and tile % 64 == 0
    base = ws(1, 1, 1)
    assert base > 0 and base % 256 == 0
    prev = 0
    for B in (1, 2, 5, 32, 65535):
        assert ws(B, 4000, 100) >= max(prev, 1)
        prev = ws(B, 4000, 100)
    prev = 0
    for L in (1, 2, tile - 1, tile, tile + 1, 2 * tile + 3, 32000, 10 ** 6):
        assert ws(4, L, 100) >= max(prev, 1)
        prev = ws(4, L, 100)
    prev = 0
    for K in (1, 2, 1000, 20000, 65536):
        assert ws(4, 4000, K) >= max(prev, 1)
        prev = ws(4, 4000, K)
    assert ws(32, 32000, 8000) >= 2 * 32 * 32000 * 8             # the float64 speech and target rows
    rejected = [(0, 10, 1), (-1, 10, 1), (65536, 10, 1), (1, 0, 1), (1, -5, 1), (1, 10, 0), (1, 10, 65537), (1, 2 ** 31 - 1, 1)]
    for B, L, K in rejected:
        assert ws(B, L, K) == 0, (B, L, K)
    # a scene without located sources needs the same bytes, on every shape walked above and the rejected ones
    walked = [(B, 4000, 100) for B in (1, 2, 5, 32, 65535)] + [(4, 4000, K) for K in (1, 2, 1000, 20000, 65536)] \
        + [(4, L, 100) for L in (1, 2, tile - 1, tile, tile + 1, 2 * tile + 3, 32000, 10 ** 6)] + [(1, 1, 1), (32, 32000, 8000)]
    for B, L, K in walked + rejected:
        assert int(lib.cmgan_scene_workspace_bytes(None, B, L, K, 0)) == ws(B, L, K), (B, L, K)


# ------------------------------------------------------------------ argument errors of the C ABI, without a handle
def _call(**over):
    """cmgan_mix with plausible, aligned, never-dereferenced pointers: every error is raised before any is followed."""
    p = 0x10000
    a = dict(h=None, clean=p, B=2, L=100, ld=100, bank=p, bank_len=50, start=p, length=p, off=p, rir=p, R=3, Kmax=16,
             idx=p, rlen=p, snr=p, peak=0.99, early=-1, noisy=p, target=p, ld_out=100, g=p, scale=p, ps=p, pn=p, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.cmgan_mix(*[a[k] for k in ("h", "clean", "B", "L", "ld", "bank", "bank_len", "start", "length", "off", "rir",
                                        "R", "Kmax", "idx", "rlen", "snr", "peak", "early", "noisy", "target", "ld_out",
                                        "g", "scale", "ps", "pn", "ws", "ws_bytes", "stream")])
    return rc, lib.cmgan_last_error(None).decode()


@pytest.mark.parametrize("over,code,text", [
    (dict(clean=None), BADARG, "null pointer"), (dict(bank=None), BADARG, "null pointer"),
    (dict(start=None), BADARG, "null pointer"), (dict(length=None), BADARG, "null pointer"),
    (dict(off=None), BADARG, "null pointer"), (dict(snr=None), BADARG, "null pointer"),
    (dict(noisy=None), BADARG, "null pointer"), (dict(target=None), BADARG, "null pointer"),
    (dict(g=None), BADARG, "null pointer"), (dict(scale=None), BADARG, "null pointer"),
    (dict(ps=None), BADARG, "null pointer"), (dict(pn=None), BADARG, "null pointer"),
    (dict(idx=None), BADARG, "rir_index and rir_len"), (dict(rlen=None), BADARG, "rir_index and rir_len"),
    (dict(clean=0x10002), BADARG, "4-byte aligned"), (dict(idx=0x10001), BADARG, "4-byte aligned"),
    (dict(start=0x10004), BADARG, "8-byte aligned"), (dict(g=0x10004), BADARG, "8-byte aligned"),
    (dict(B=0), BADARG, "B=0"), (dict(B=65536), BADARG, "B=65536"), (dict(L=0), BADARG, "L=0"),
    (dict(ld=99), BADARG, "ld=99"), (dict(ld_out=99), BADARG, "ld_out=99"), (dict(bank_len=0), BADARG, "bank_len=0"),
    (dict(peak=0.0), BADARG, "peak"), (dict(peak=-1.0), BADARG, "peak"), (dict(peak=float("nan")), BADARG, "peak"),
    (dict(peak=float("inf")), BADARG, "peak"), (dict(early=-2), BADARG, "early"),
    (dict(R=0), BADARG, "R=0"), (dict(Kmax=0), BADARG, "Kmax=0"),
    (dict(Kmax=65537), UNSUPPORTED, "65536 taps"),
    (dict(L=2 ** 31 - 1, ld=2 ** 31 - 1, ld_out=2 ** 31 - 1), UNSUPPORTED, "samples are supported"),
    (dict(), BADARG, "null handle"),                              # everything valid: only now is the handle missed
    (dict(rir=None, R=0, Kmax=0, idx=None, rlen=None), BADARG, "null handle"),     # no bank: R / Kmax are not looked at
])
def test_abi_argument_errors_without_gpu(over, code, text):
    rc, msg = _call(**over)
    assert rc == code, (rc, msg)
    assert msg.startswith("cmgan_mix: ") and text in msg, msg


# ------------------------------------------------------------------ argument errors of Engine.mix, on CPU tensors
def _args(B=3, L=50, R=2, K=8):
    return dict(clean=torch.zeros(B, L), noise_bank=torch.zeros(40), noise_start=torch.zeros(B, dtype=torch.int64),
                noise_len=torch.ones(B, dtype=torch.int64), noise_off=torch.zeros(B, dtype=torch.int64),
                snr_db=torch.zeros(B), rir_bank=torch.zeros(R, K), rir_index=torch.zeros(B, dtype=torch.int32),
                rir_len=torch.ones(B, dtype=torch.int32))


def test_engine_mix_argument_rules_without_gpu():
    cpu = torch.device("cpu")
    assert check_mix_args(cpu, **_args()) == (3, 50, 2, 8)
    a = _args()
    a.update(rir_bank=None, rir_index=None, rir_len=None)
    assert check_mix_args(cpu, **a) == (3, 50, 0, 0)
    cases = [
        (dict(clean=torch.zeros(50)), ValueError, "clean"), (dict(clean=torch.zeros(3, 0)), ValueError, "clean"),
        (dict(clean=torch.zeros(3, 50, dtype=torch.float64)), TypeError, "clean"),
        (dict(clean=np.zeros((3, 50), np.float32)), TypeError, "clean"),
        (dict(clean=torch.zeros(50, 3).t()), ValueError, "contiguous"),
        (dict(noise_bank=torch.zeros(4, 10)), ValueError, "noise_bank"), (dict(noise_bank=torch.zeros(0)), ValueError, "noise_bank"),
        (dict(noise_start=torch.zeros(3, dtype=torch.int32)), TypeError, "noise_start"),
        (dict(noise_len=torch.ones(4, dtype=torch.int64)), ValueError, "noise_len"),
        (dict(noise_off=torch.zeros(3)), TypeError, "noise_off"),
        (dict(snr_db=torch.zeros(3, dtype=torch.float64)), TypeError, "snr_db"), (dict(snr_db=torch.zeros(1)), ValueError, "snr_db"),
        (dict(rir_bank=torch.zeros(8)), ValueError, "rir_bank"),
        (dict(rir_bank=torch.zeros(1, MIX_MAX_TAPS + 1)), ValueError, "taps"),
        (dict(rir_index=None), ValueError, "rir_index and rir_len"), (dict(rir_len=None), ValueError, "rir_index and rir_len"),
        (dict(rir_index=torch.zeros(3, dtype=torch.int64)), TypeError, "rir_index"),
        (dict(rir_len=torch.ones(2, dtype=torch.int32)), ValueError, "rir_len"),
        (dict(rir_bank=None), ValueError, "without a rir_bank"),
        (dict(peak=0.0), ValueError, "peak"), (dict(peak=float("inf")), ValueError, "peak"), (dict(peak=float("nan")), ValueError, "peak"),
        (dict(early=-2), ValueError, "early"), (dict(early=1.5), ValueError, "early"),
    ]
    for over, exc, text in cases:
        a = _args()
        a.update(over)
        with pytest.raises(exc, match=text):
            check_mix_args(cpu, **a)
    with pytest.raises(RuntimeError, match="bound to"):
        check_mix_args(torch.device("meta"), **_args())


def test_banks_keep_one_allocation_and_index_tables():
    from cmgan_amd.mixing import NoiseBank, RirBank
    nb = NoiseBank.from_arrays([np.arange(5.0), np.arange(3.0) + 10, [7.0]])
    assert len(nb) == 3 and nb.data.dtype == torch.float32 and nb.data.tolist() == [0, 1, 2, 3, 4, 10, 11, 12, 7]
    assert nb.start.dtype == nb.length.dtype == torch.int64
    assert nb.start.tolist() == [0, 5, 8] and nb.length.tolist() == [5, 3, 1]
    rb = RirBank.from_arrays([[1.0, 0.5], [0.1, 0.9, 0.3, 0.2]])
    assert tuple(rb.data.shape) == (2, 4) and rb.length.dtype == torch.int32 and rb.length.tolist() == [2, 4]
    assert rb.data[0].tolist() == [1.0, 0.5, 0.0, 0.0]
    ri = rb.with_identity()
    assert tuple(ri.data.shape) == (3, 4) and ri.data[2].tolist() == [1.0, 0, 0, 0] and ri.length.tolist() == [2, 4, 1]
    with pytest.raises(ValueError):
        NoiseBank.from_arrays([])
    with pytest.raises(ValueError):
        NoiseBank.from_arrays([np.zeros((2, 2))])


def test_clean_only_dataset_follows_the_length_rule(tmp_path):
    from scipy.io import wavfile
    from cmgan_amd.data import fit_length
    from cmgan_amd.mixing import clean_only
    d = tmp_path / "clean"
    os.makedirs(d)
    rng = np.random.default_rng(0)
    short = (rng.standard_normal(30) * 3000).astype(np.int16)
    long_ = (rng.standard_normal(200) * 3000).astype(np.int16)
    wavfile.write(d / "a2.wav", 16000, long_)
    wavfile.write(d / "a10.wav", 16000, short)
    ds = clean_only(str(tmp_path), cut_len=64)
    assert len(ds) == 2 and ds.clean_wav_name == ["a2.wav", "a10.wav"]
    x, n = ds[1]
    assert n == 30 and torch.equal(x, fit_length(torch.from_numpy(short.astype(np.float32) / 32768.0), 64))
    x, n = ds[0]
    full = long_.astype(np.float32) / 32768.0
    assert n == 200 and x.numel() == 64
    assert any(np.array_equal(x.numpy(), full[s:s + 64]) for s in range(200 - 64 + 1))


# ------------------------------------------------------------------ DynamicMixer's draws and messages, as recorded
def test_draws_and_messages_are_the_recorded_ones():
    """DynamicMixer's contract is exact - draw order, generator state, bits, and the text of every refusal - so both are
    pinned from outside (tests/golden/make_mixer_draws.py, recorded at the commit before the constructor and the draws
    were rebuilt from shared helpers): for the 384 option combinations of tests/mixer_cases.py every field of draw(6) and
    draw_stretch(6, d.speed) - dtype, shape, strides and bits, None where it was None - and the final state of the three
    generators; for one bad option per parser path, and for pairs of them, the exception type and its full text."""
    import json
    import mixer_cases as C
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(golden, "mixer_parent_draws.npz"))
    manifest, blob = json.loads(str(z["manifest"])), z["blob"]
    redo = (f"; recorded at {str(z['provenance'])!r}, this is torch {torch.__version__}: if torch's generators moved, record "
            f"again with tests/golden/make_mixer_draws.py AT THAT COMMIT, not at the one under test")
    cases = list(C.draw_cases())
    assert len(cases) == 384 and [name for name, _ in cases] == list(manifest)
    at = 0
    for name, opt in cases:
        mixer, gens = C.draw_mixer(opt, C.NoEngine())
        rows, raw = C.pack(C.drawn_fields(mixer, gens))
        assert [r[0] for r in rows] == [w[0] for w in manifest[name]], f"{name}: fields {[r[0] for r in rows]}" + redo
        mine = 0
        for got, want in zip(rows, manifest[name]):
            assert got == want, f"{name} {got[0]}: [name, dtype, shape, strides, bytes] = {got}, recorded {want}" + redo
            n = 0 if want[1] is None else want[-1]
            if not np.array_equal(raw[mine:mine + n], blob[at:at + n]):
                k = int(np.argmax(raw[mine:mine + n] != blob[at:at + n]))
                raise AssertionError(f"{name} {got[0]} ({got[1]} {got[2]}): differs first at byte {k}" + redo)
            mine, at = mine + n, at + n
    assert at == blob.size
    with open(os.path.join(golden, "mixer_parent_messages.json")) as f:
        recorded = json.load(f)["messages"]
    assert list(recorded) == [name for name, _, _ in C.BAD_OPTIONS]
    for name, make, kw in C.BAD_OPTIONS:
        assert C.message_of(make, kw) == recorded[name], f"{name}: {make.__name__}({kw})"
