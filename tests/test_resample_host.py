"""CPU side of the GPU resampler (cmgan_amd/csrc/resample.hip): the tap table exported through cmgan_resample_table
from the same C++ code as the table kernel, against scipy's construction; the geometry and length formulas; the numpy
model of the kernel's sum (tests/resample_model.py) against scipy.signal.resample_poly; and the Resampler's host
bookkeeping replayed on index arrays."""
import ctypes

import numpy as np
import pytest
from scipy import signal as sig

import resample_model as RM
from cmgan_amd import _lib
from cmgan_amd.resample import ResamplePlan, geometry, out_len

TOL = 1e-13          # tests/test_metrics_tables.py's tolerance for the same construction
PAIRS = RM.PAIRS


def table(fs_in, fs_out):
    lib = _lib.load()
    n = lib.cmgan_resample_table(fs_in, fs_out, None, 0)
    assert n > 0, n
    out = np.full(n, np.nan)
    assert lib.cmgan_resample_table(fs_in, fs_out, out.ctypes.data_as(ctypes.c_void_p), n) == n
    return out


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_tap_table_matches_scipy_construction(fs_in, fs_out):
    up, down, n_taps, _ = RM.geometry(fs_in, fs_out)
    m = max(up, down)
    h = sig.firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    want = np.concatenate([np.zeros(down - (10 * m) % down), h])
    got = table(fs_in, fs_out)
    assert got.shape == want.shape == (n_taps,)
    err = np.max(np.abs(got - want))
    print(f"{fs_in}->{fs_out}: {n_taps} taps, max |got - scipy| = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_geometry_and_length_equal_the_formulas(fs_in, fs_out):
    assert tuple(geometry(fs_in, fs_out)) == RM.geometry(fs_in, fs_out)
    up, down, _, _ = RM.geometry(fs_in, fs_out)
    for L in (0, 1, 2, 255, 256, 257, 32000, 88200, 2 ** 31 - 1):
        assert out_len(fs_in, fs_out, L) == -(-L * up // down)
    for L in (1, 7, 255, 4411, 88201):                               # a round trip never loses samples
        assert out_len(fs_out, fs_in, out_len(fs_in, fs_out, L)) >= L


def test_table_sizes_of_the_contract():
    assert RM.geometry(44100, 16000)[2] == 9262 and -(-9262 // 160) == 58
    assert RM.geometry(11025, 16000)[2] == 13016
    assert RM.geometry(48000, 16000)[2] == 64


def test_unsupported_pairs_and_argument_errors_without_gpu():
    lib = _lib.load()
    i = ctypes.c_int()
    assert lib.cmgan_resample_geometry(16000, 44101, ctypes.byref(i), None, None, None) == -3    # CMGAN_E_UNSUPPORTED
    assert b"44101" in lib.cmgan_last_error(None)
    assert lib.cmgan_resample_geometry(0, 16000, None, None, None, None) == -3
    assert lib.cmgan_resample_table(16000, 44101, None, 0) == -3
    assert lib.cmgan_resample_out_len(16000, 44101, 100) == -3
    assert lib.cmgan_resample_out_len(16000, 8000, -1) == -1                                     # CMGAN_E_BADARG
    assert lib.cmgan_resample_workspace_bytes(None, 16000, 44101) == 0
    assert lib.cmgan_resample_workspace_bytes(None, 44100, 16000) >= 160 * 58 * 8
    small = np.zeros(4)
    assert lib.cmgan_resample_table(48000, 16000, small.ctypes.data_as(ctypes.c_void_p), small.size) == -1
    assert lib.cmgan_resample(None, None, 1, 10, 10, 0, 48000, 16000, 0, 4, None, 4, None, 0, None) == -1
    # the largest supported ratio: 640, a table of 13 441 doubles with its pre-pad
    assert lib.cmgan_resample_geometry(640, 1, None, None, None, None) == 0
    assert lib.cmgan_resample_table(1, 640, None, 0) == 12802
    assert lib.cmgan_resample_table(640, 1, None, 0) == 13441
    assert lib.cmgan_resample_geometry(641, 1, None, None, None, None) == -3
    with pytest.raises(_lib.CmganError):
        geometry(16000, 44101)


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_model_equals_scipy_resample_poly(fs_in, fs_out):
    """The contract's sum (plain loop, and its per-phase form on a longer clip) against scipy on float64 copies of float32
    noise, odd lengths: 1e-13 of the peak (measured: about 2e-15)."""
    up, down, _, _ = RM.geometry(fs_in, fs_out)
    rng = np.random.default_rng(fs_in + fs_out)
    for L, model in ((1, RM.resample), (301, RM.resample), (4411, RM.resample_fast)):
        x = rng.standard_normal(L).astype(np.float32).astype(np.float64)
        want = sig.resample_poly(x, up, down)
        got = model(x, fs_in, fs_out)
        assert got.shape == want.shape == (RM.out_len(fs_in, fs_out, L),)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"{fs_in}->{fs_out} L={L}: max err / peak = {err:.3e}")
        assert err <= 1e-13
    # a chunk of the model: outputs [n0, n0 + n) from a buffer that holds just the inputs they reach
    x = rng.standard_normal(997).astype(np.float32).astype(np.float64)
    whole = RM.resample(x, fs_in, fs_out)
    plan = ResamplePlan(*RM.geometry(fs_in, fs_out))
    n0, n = whole.size // 3, min(40, whole.size - whole.size // 3)
    lo, hi = plan.first_input(n0), min(plan.last_input(n0 + n - 1), x.size - 1)
    assert np.array_equal(RM.resample(x[lo:hi + 1], fs_in, fs_out, n0=n0, n_out=n, pos_in=lo), whole[n0:n0 + n])


def _chunkings(rng, L, longest):
    yield [1] * min(L, 300) + ([L - 300] if L > 300 else [])
    yield [L]
    for _ in range(3):
        sizes, left = [], L
        while left:
            n = int(min(left, rng.choice([1, 2, 3, 17, 160, 441, 1000, longest])))
            sizes.append(n)
            left -= n
        yield sizes


@pytest.mark.parametrize("fs_in,fs_out", PAIRS + [(16000, 16000)])
def test_chunk_plan_emits_every_output_once_in_order_and_keeps_what_they_reach(fs_in, fs_out):
    """ResamplePlan replayed on input INDEX arrays: the buffer is the array of indices held.  Chunks of 1 sample and chunks
    longer than the tap table are included."""
    geom = RM.geometry(fs_in, fs_out) if fs_in != fs_out else (1, 1, 1, 0)
    up, down, n_taps, pre_remove = geom
    rng = np.random.default_rng(7 * fs_in + fs_out)
    L = 2 * n_taps + 1237
    N = -(-L * up // down)
    ref = ResamplePlan(*geom)
    for sizes in _chunkings(rng, L, n_taps + 50):
        plan = ResamplePlan(*geom)
        held = np.empty(0, dtype=np.int64)
        emitted, arrived = [], 0
        for step, n_new in enumerate(sizes + [0]):
            last = step == len(sizes)
            held = np.concatenate([held, np.arange(arrived, arrived + n_new)])
            arrived += n_new
            p = plan.plan(n_new, last)
            assert p["pos_in"] == (held[0] if held.size else arrived) and p["n_buf"] == held.size
            for n in range(p["n0"], p["n0"] + p["n_out"]):
                lo, hi = ref.first_input(n), ref.last_input(n)
                assert last or hi < arrived, f"output {n} emitted before its last input {hi}"
                need = np.arange(lo, min(hi, L - 1) + 1)
                assert need.size == 0 or (need[0] >= held[0] and need[-1] <= held[-1]), f"output {n}: input dropped"
                emitted.append(n)
            held = held[p["drop"]:]
            plan.commit(p)
            if not last:                                             # nothing the coming outputs reach is kept in vain
                assert held.size == 0 or held[0] == min(ref.first_input(plan.n_out), arrived)
        assert emitted == list(range(N)), "every output exactly once and in order"
        with pytest.raises(RuntimeError):
            plan.plan(1)
