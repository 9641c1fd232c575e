"""CPU side of the active speech level (cmgan_amd/csrc/level.hip; include/cmgan_hip.h, "Active speech level"): the
float64 model the GPU tests compare the kernels with (tests/level_model.py) against its own definition as a naive loop
with hangover counters, the tile decomposition the kernels use against the sequential loop, known answers, the workspace
formula, and every argument error of cmgan_speech_level, Engine.speech_level and DynamicMixer(snr_on=, level_db=), all of
which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import level_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import LEVEL_MAX_L, LEVEL_TILE, check_level_args, level_workspace_bytes
from cmgan_amd.mixing import DynamicMixer, NoiseBank

BADARG = -1
CPU = torch.device("cpu")


# ------------------------------------------------------------------ the model against the definition as a loop
def _naive_counts(x, fs):
    """Per sample and threshold: a hit counts and re-arms the hangover, a miss counts while the hangover lasts."""
    g, hang = M.constants(fs)
    a, h = [0] * 15, [hang] * 15
    p = q = 0.0
    for v in np.abs(np.asarray(x, dtype=np.float64)).tolist():
        p = g * p + (1.0 - g) * v
        q = g * q + (1.0 - g) * p
        for j in range(15):
            if q >= M.THRESHOLDS[j]:
                a[j] += 1
                h[j] = 0
            elif h[j] < hang:
                a[j] += 1
                h[j] += 1
    return a


@pytest.mark.parametrize("seed,fs,L", [(1, 8000, 4000), (2, 8000, 5203), (3, 16000, 7001)])
def test_model_counts_equal_the_naive_hangover_loop(seed, fs, L):
    x = M.bursts(seed, L, fs=fs)
    ms, active, frac, counts, q = M.level(x, L, fs)
    assert counts[:15].tolist() == _naive_counts(x, fs) and counts[15] == L
    assert counts[0] > 0 and counts[14] < counts[0]                  # the signal spreads over the thresholds
    assert all(counts[j] >= counts[j + 1] for j in range(14))
    assert 0.0 < frac <= 1.0 and active >= ms > 0.0


def test_model_hangover_is_I_samples_after_the_last_crossing():
    fs = 8000
    g, hang = M.constants(fs)
    x = np.zeros(4000)
    x[:400] = 0.5
    q = M.envelope(x, fs)
    last = int(np.nonzero(q >= M.THRESHOLDS[10])[0][-1])
    first = int(np.nonzero(q >= M.THRESHOLDS[10])[0][0])
    assert M.activity_counts(q, fs)[10] == last + hang + 1 - first
    assert M.activity_counts(q[:last + hang], fs)[10] == last + hang - first      # cut one sample short of the hangover's end


# ------------------------------------------------------------------ the tile decomposition of the kernels
def _tiled_envelope(x, fs, tile, run):
    """q by the kernels' decomposition: runs of `run` samples from zero state, segments composed as
    p' = g^m p + P, q' = g^m q + m (1-g) g^m p + Q inside a tile and from tile to tile, then every run from its entry state."""
    g, _ = M.constants(fs)
    omg, tau = 1.0 - g, 0.03 * fs
    gp = lambda m: math.exp(-m / tau)
    n = len(x)
    nt = -(-n // tile)
    xa = np.zeros(nt * tile)
    xa[:n] = np.abs(x)

    def from_zero(seg, p=0.0, q=0.0):
        out = []
        for v in seg.tolist():
            p = g * p + omg * v
            q = g * q + omg * p
            out.append(q)
        return p, q, out

    def compose(A, B, m):                     # segment A, then segment B of m samples
        gm = gp(m)
        return gm * A[0] + B[0], gm * A[1] + m * omg * gm * A[0] + B[1]

    q_all = np.zeros(nt * tile)
    state = (0.0, 0.0)
    for k in range(nt):
        t0 = k * tile
        runs = [from_zero(xa[t0 + r:t0 + r + run])[:2] for r in range(0, tile, run)]
        prefix = (0.0, 0.0)                   # the runs before the current one, from zero state
        for r, seg in enumerate(runs):
            m = r * run
            gm = gp(m)
            entry = (gm * state[0] + prefix[0], gm * state[1] + m * omg * gm * state[0] + prefix[1])
            q_all[t0 + m:t0 + m + run] = from_zero(xa[t0 + m:t0 + m + run], *entry)[2]
            prefix = compose(prefix, seg, run)
        state = compose(state, prefix, tile)
    return q_all[:n]


@pytest.mark.parametrize("fs", [8000, 16000])
def test_tile_composition_equals_the_sequential_loop(fs):
    x = M.bursts(11, 3 * 1024 + 77, fs=fs).astype(np.float64)
    q = M.envelope(x, fs)
    qt = _tiled_envelope(x, fs, 1024, 4)
    err = float(np.max(np.abs(q - qt)))
    top = float(np.max(np.abs(x)))
    print(f"[level] fs={fs}: tile form vs sequential loop {err:.2e} at max|x| = {top}")
    assert err <= M.guard_delta(fs) * top / 8                         # well inside the guard the GPU tests rely on
    assert M.guard_delta(fs) == 2.0 ** -40


def test_guard_counts_decisions_within_reach_of_rounding():
    fs = 8000
    x = M.bursts(1, 3000, fs=fs)
    _, _, _, counts, q = M.level(x, 3000, fs)
    assert M.guard_hits(q, x, counts, fs) == 0
    q2 = q.copy()
    q2[1234] = M.THRESHOLDS[7] * (1.0 + 1e-15)
    q2[77] = M.THRESHOLDS[3]
    assert M.guard_hits(q2, x, counts, fs) == 2
    assert M.guard_delta(192000) > 2.0 ** -40                         # widened by the derivation, not by a measurement


# ------------------------------------------------------------------ known answers
def test_silent_and_sub_threshold_rows_give_zeros():
    fs, L = 16000, 5000
    for x in (np.zeros(L), np.full(L, 2.0 ** -16 * 0.999), -np.full(L, 1e-6)):
        ms, active, frac, counts, _ = M.level(x, L, fs)
        assert (ms, active, frac) == (0.0, 0.0, 0.0)
        assert counts.tolist() == [0] * 15 + [L]
    assert M.level(np.ones(10), 0, fs)[:3] == (0.0, 0.0, 0.0)


def test_steady_tone_is_all_active():
    """The envelope needs some 25 ms to rise through the threshold that decides (1.2 % of a 2 s row): 40 s make it 0.06 %."""
    fs, L = 16000, 640000
    x = 0.25 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / fs)
    ms, active, frac, counts, _ = M.level(x, L, fs)
    assert abs(active / 0.03125 - 1.0) < 1e-3
    assert frac > 0.99
    assert abs(ms / 0.03125 - 1.0) < 1e-3


def test_tone_bursts_count_the_hangover_as_active_time():
    fs, L = 16000, 64000
    i = np.arange(L)
    x = 0.25 * np.sin(2 * np.pi * 1000.0 * i / fs) * ((i // fs) % 2 == 0)
    ms, active, frac, _, _ = M.level(x, L, fs)
    assert abs(frac - 0.638) < 1e-3
    assert abs(active - 0.02448) < 1e-5
    assert abs(ms - 0.015625) < 1e-6


def test_non_finite_row_gives_nans():
    x = np.full(100, 0.1)
    x[40] = np.inf
    assert all(math.isnan(v) for v in M.level(x, 100, 16000)[:3])


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_speech_level", "cmgan_speech_level_workspace_bytes", "cmgan_speech_level_tile"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_speech_level_tile() == LEVEL_TILE
    assert LEVEL_TILE <= 8000 // 5 + 1                                # no longer than the shortest hangover + 1
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 9


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda B, L: int(lib.cmgan_speech_level_workspace_bytes(B, L))
    for B in (1, 2, 5, 32, 65535):
        for L in (1, 1023, 1024, 1025, 32000, 160000, LEVEL_MAX_L):
            assert ws(B, L) == level_workspace_bytes(B, L) > 0 and ws(B, L) % 256 == 0, (B, L)
    assert ws(3, 32000) <= ws(4, 32000) and ws(4, 32000) <= ws(4, 32001 + 1024)
    for B, L in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, -5), (1, LEVEL_MAX_L + 1)):
        assert ws(B, L) == level_workspace_bytes(B, L) == 0, (B, L)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(4096, dtype=np.float32)
    lengths = np.zeros(8, dtype=np.int32)
    level = np.zeros(64, dtype=np.float64)
    counts = np.zeros(64, dtype=np.int64)
    raw = np.zeros(1 << 16, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    px, pl, pv, pc = x.ctypes.data, lengths.ctypes.data, level.ctypes.data, counts.ctypes.data

    def call(x=px, B=2, L=1500, ld=1500, lengths=pl, fs=16000, level=pv, counts=pc, ws=base, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = level_workspace_bytes(B, L) if 1 <= B <= 8 and 1 <= L <= 2048 else 4096
        rc = lib.cmgan_speech_level(None, x, B, L, ld, lengths, fs, level, counts, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(x=None), dict(level=None)],
        "aligned": [dict(x=px + 2), dict(lengths=pl + 1), dict(level=pv + 4), dict(counts=pc + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(ld=1499)],
        "rows of up to": [dict(L=LEVEL_MAX_L + 1, ld=2 ** 31 - 1)],
        "fs must lie": [dict(fs=7999), dict(fs=192001), dict(fs=0), dict(fs=-16000)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=level_workspace_bytes(2, 1500) - 1), dict(ws_bytes=0)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(counts=None), dict(fs=8000), dict(fs=192000)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not level.any() and not counts.any()


# ------------------------------------------------------------------ Engine.speech_level's argument rules
def test_check_level_args():
    ok = torch.zeros(3, 2000)
    assert check_level_args(CPU, ok) == (3, 2000)
    assert check_level_args(CPU, ok, torch.zeros(3, dtype=torch.int32), 8000) == (3, 2000)
    assert check_level_args(CPU, torch.zeros(3, 2500)[:, :2000], None, 192000) == (3, 2000)      # a row stride larger than L
    assert check_level_args(CPU, torch.zeros(1, 7)) == (1, 7)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_level_args(CPU, np.zeros((3, 2000), dtype=np.float32))
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_level_args(CPU, ok.double())
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_level_args(torch.device("cuda:0"), ok)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_level_args(CPU, bad)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_level_args(CPU, torch.zeros(1, 1).expand(65536, 1))
    with pytest.raises(ValueError, match="rows must be contiguous"):
        check_level_args(CPU, torch.zeros(3, 4000)[:, ::2])
    with pytest.raises(ValueError, match="rows must be contiguous"):
        check_level_args(CPU, torch.zeros(2000, 3).t())
    with pytest.raises(ValueError, match="rows must be contiguous"):
        check_level_args(CPU, torch.zeros(1, 2000).expand(3, 2000))
    with pytest.raises(TypeError, match="lengths: expected int32"):
        check_level_args(CPU, ok, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError, match="lengths: expected a torch.Tensor"):
        check_level_args(CPU, ok, [1, 2, 3])
    with pytest.raises(ValueError, match="lengths: expected \\[3\\]"):
        check_level_args(CPU, ok, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="lengths: must be contiguous"):
        check_level_args(CPU, ok, torch.zeros(6, dtype=torch.int32)[::2])
    for fs in (7999, 192001, 16000.5, 0, True):
        with pytest.raises(ValueError, match="fs must be a sample rate"):
            check_level_args(CPU, ok, None, fs)


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def test_mixer_rejects_bad_level_options():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32)])
    with pytest.raises(ValueError, match="snr_on must be 'rms' or 'active'"):
        DynamicMixer(_NoEngine(), bank, snr_on="peak")
    with pytest.raises(ValueError, match="level_db must be \\(low, high\\)"):
        DynamicMixer(_NoEngine(), bank, level_db=(-15.0, -35.0))
    with pytest.raises(ValueError, match="level_db must be"):
        DynamicMixer(_NoEngine(), bank, level_db=-20.0)
    with pytest.raises(ValueError, match="level_db must be"):
        DynamicMixer(_NoEngine(), bank, level_db=(-math.inf, -20.0))
    with pytest.raises(ValueError, match="8000 .. 192000 Hz"):
        DynamicMixer(_NoEngine(), bank, snr_on="active", sample_rate=4000)
    m = DynamicMixer(_NoEngine(), bank)
    assert m.snr_on == "rms" and m.level_db is None and m.last_level is None
    m = DynamicMixer(_NoEngine(), bank, snr_on="active", level_db=(-35, -15))
    assert m.snr_on == "active" and m.level_db == (-35.0, -15.0)
    DynamicMixer(_NoEngine(), bank, sample_rate=4000)                  # the defaults measure nothing: any rate, as before


def test_default_draw_has_no_level():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])
    gen = lambda: torch.Generator().manual_seed(7)
    d0 = DynamicMixer(_NoEngine(), bank, generator=gen()).draw(6)
    d1 = DynamicMixer(_NoEngine(), bank, generator=gen(), snr_on="active").draw(6)
    d2 = DynamicMixer(_NoEngine(), bank, generator=gen(), level_db=(-35, -15)).draw(6)
    assert d0.level_db is None and d1.level_db is None
    for a, b, c in zip(d0[:4], d1[:4], d2[:4]):                      # the new draw comes after all the others
        assert torch.equal(a, b) and torch.equal(a, c)
    assert d2.level_db.dtype == torch.float64 and tuple(d2.level_db.shape) == (6,)
    assert bool(((d2.level_db >= -35) & (d2.level_db <= -15)).all())
