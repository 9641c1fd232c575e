"""GPU tests of the intelligibility loss (cmgan_amd/csrc/stoiloss.hip: Engine.stoi_loss, Engine.estoi, the `w_stoi` term of
training.AuxLoss) against the numpy model of tests/stoiloss_model.py, whose docstring states the acceptance rule and the
two margins; tests/test_stoiloss_host.py checks, without a GPU, that every case meets them.

Two batches of four rows.  L = 9600 (45 frames at 10 kHz): (a) a noisy estimate of a voiced row, (c) est == ref bit for
bit, (d) a reference that keeps exactly 31 frames (one window), (e) one that keeps 30 (status bit 0).  L = 16000 (77 frames):
(b) a reference with 0.25 s of near-silence in the middle, whose kept frames straddle the gap, (f) an all-zero estimate
(status bit 1), a noisy speech-like row with pauses of its own, and (b) again.

Measured on an MI355X over every judged row: the STOI value is EQUAL to Engine.metrics' (one body in stoi_common.hip.h is
behind both kernels' sums, so the assertion is equality of the float64 bits); the worst value
error against the long-double model is 7.2e-15 (bound 6.0e-13); no gradient sample of a noisy row lies beyond half an ulp of
the long-double value (excess 0 of E), and on (c), whose true gradient is 0, the worst excess is 0.10 of E."""
import numpy as np
import pytest
import torch

import stoiloss_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = M.K_WEIGHT


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_same(x, y):
    return all((p is None and q is None) or _same_bits(p, q) for p, q in zip(x, y))


# ------------------------------------------------------------------ values and gradients
@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("L", [M.L_SHORT, M.L_LONG])
def test_values_and_gradients_against_the_model(eng, L, extended):
    est, ref, names = M.batch(L)
    k = W / len(names)
    models = [M.row_model(M.registered(n), extended, k) for n in names]
    for n, m in zip(names, models):                                     # the conditions, before anything is compared
        assert m.level_margin >= M.LEVEL_MARGIN and m.min_margin >= M.MIN_MARGIN, (n, m.level_margin, m.min_margin)
    d_est, d_ref = _dev(est, ref)
    out = eng.stoi_loss(d_est, d_ref, W, extended)
    assert out.rows.dtype == torch.float64 and tuple(out.rows.shape) == (4, 2) and out.status.dtype == torch.int32
    assert out.total.dtype == torch.float32 and tuple(out.total.shape) == (1,) and tuple(out.grad.shape) == (4, L)
    rows, status, grad = out.rows.cpu().numpy(), out.status.cpu().numpy(), out.grad.cpu().numpy()
    metric = None if extended else eng.metrics(d_ref, d_est).stoi.cpu().numpy()
    want_total, slack = M.LD(0), 0.0
    for b, (n, m) in enumerate(zip(names, models)):
        assert int(rows[b, 1]) == m.kept and int(status[b]) == m.status, (n, rows[b], status[b], m.kept, m.status)
        if m.status:
            assert np.isnan(rows[b, 0]) and not grad[b].any(), n     # NaN, left out of the total, exact zeros
            assert metric is None or np.isnan(metric[b])
            continue
        err = float(abs(M.LD(rows[b, 0]) - m.value))
        ok, frac = M.accept(grad[b], m)
        line = f"[stoiloss] L={L} extended={extended} case {n}: value error = {err:.2e} (bound {m.bound:.2e}), gradient excess = {frac:.3f} of E"
        if metric is not None:
            line += f", |value - Engine.metrics| = {abs(rows[b, 0] - metric[b]):.2e} ({'equal' if rows[b, 0] == metric[b] else 'not equal'})"
        print(line)
        assert err <= m.bound, (n, err, m.bound)
        if metric is not None:
            assert rows[b, 0].view(np.int64) == metric[b].view(np.int64), (n, rows[b, 0], metric[b])
        assert ok, (n, frac, m.E)
        want_total += m.a
        slack += k * m.bound
    got = float(out.total[0])
    assert abs(M.LD(got) - want_total) <= M.ulp32(float(want_total)) / 2 + slack + 8 * M.U * abs(float(want_total)), (got, float(want_total))
    if L == M.L_SHORT:
        assert abs(rows[names.index("c"), 0] - 1.0) <= 1e-14
    # the scorer
    if extended:
        sc = eng.estoi(d_ref, d_est)
        assert sc.dtype == torch.float64 and tuple(sc.shape) == (4,) and _same_bits(sc, out.rows[:, 0].contiguous())


# ------------------------------------------------------------------ reproducibility, independence, capture
@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_reproducible_values_alone_not_in_place_and_capturable(eng, extended):
    L = M.L_SHORT
    est, ref, names = M.batch(L)
    est, ref = _dev(est, ref)
    a = eng.stoi_loss(est, ref, W, extended)
    b = eng.stoi_loss(est, ref, W, extended)
    assert _all_same(a, b)
    s = eng.stoi_loss(est, ref, W, extended, grad=False)
    assert s.grad is None and _same_bits(s.rows, a.rows) and _same_bits(s.total, a.total) and _same_bits(s.status, a.status)
    # the gradient is never formed in place: refused before anything is launched
    scratch = est.clone()
    ws = eng._wss["stoi_loss"]
    rows, total, status = torch.full_like(a.rows, 7.0), torch.full_like(a.total, 7.0), torch.full_like(a.status, 7)
    rc = eng.lib.cmgan_stoi_loss(eng._h, scratch.data_ptr(), ref.data_ptr(), 4, L, 16000, int(extended), W / 4, rows.data_ptr(),
                                 total.data_ptr(), status.data_ptr(), scratch.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"g_audio overlaps" in eng.lib.cmgan_last_error(eng._h)
    assert torch.equal(scratch, est) and bool((rows == 7.0).all()) and bool((total == 7.0).all()) and bool((status == 7).all())
    # captured and replayed on new contents of the static inputs (other kept-frame counts than at the capture)
    se, sr = torch.ones_like(est), torch.ones_like(ref).mul_(0.5)
    se[:, ::2] = -1.0
    sr[:, ::3] = -0.5
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = eng.stoi_loss(se, sr, W, extended)
    se.copy_(est)
    sr.copy_(ref)
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(got, a)


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_a_row_has_the_bits_it_has_alone_and_beside_other_neighbours(eng, extended):
    L = M.L_SHORT
    est, ref, names = M.batch(L)
    est, ref = _dev(est, ref)
    out = eng.stoi_loss(est, ref, W, extended)
    ia = names.index("a")
    one = eng.stoi_loss(est[ia:ia + 1].contiguous(), ref[ia:ia + 1].contiguous(), W / 4, extended)      # the same k
    assert _same_bits(one.rows[0], out.rows[ia]) and _same_bits(one.grad[0], out.grad[ia]) and _same_bits(one.status, out.status[ia:ia + 1])
    order = [3, 2, 0, 1]                                                # other neighbours, another place in the batch
    mixed = eng.stoi_loss(est[order].contiguous(), ref[order].contiguous(), W, extended)
    for new, old in enumerate(order):
        assert _same_bits(mixed.rows[new], out.rows[old]) and _same_bits(mixed.grad[new], out.grad[old]), (new, old)
    assert _same_bits(mixed.status, out.status[order].contiguous())
    # a NaN beside it stays in its own row, which gets a status and leaves the total
    e2 = est.clone()
    e2[1, 777] = float("nan")
    bad = eng.stoi_loss(e2, ref, W, extended)
    assert int(bad.status[1]) == 2 and bool(torch.isnan(bad.rows[1, 0])) and not bool(bad.grad[1].any())
    assert _same_bits(bad.rows[ia], out.rows[ia]) and _same_bits(bad.grad[ia], out.grad[ia]) and bool(torch.isfinite(bad.total).all())


# ------------------------------------------------------------------ wiring into the training step
TRAIN_L = 6600       # the shortest multiple of the hop that holds 31 frames at 10 kHz: B x T = 1 x 67, the work of the 2 x 33 that
                     # tests/test_gpu_training.py steps at (its own L = 3200 is below what STOI is defined for)


@pytest.fixture(scope="module")
def clips():
    from cmgan_amd.synth import synthetic_clips
    clean = synthetic_clips(1, TRAIN_L, seed=5).to(DEV)
    noisy = (clean + 0.3 * synthetic_clips(1, TRAIN_L, seed=6).to(DEV)).contiguous()
    return clean, noisy


def _fresh():
    from cmgan_amd.training import AdamW, GeneratorTrain
    from oracle.weights import make_state_dict
    gen = GeneratorTrain(make_state_dict(seed=0), device=DEV)
    return gen, AdamW(gen.engine, gen.param_bucket, gen.grad_bucket, lr=5e-4)


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_generator_train_step_with_w_stoi_is_the_manual_composition(clips, extended):
    from cmgan_amd.training import AuxLoss, generator_loss_terms, generator_train_step
    clean, noisy = clips
    B = clean.shape[0]
    w = (0.1, 0.9, 0.2)
    gen, opt = _fresh()
    eng = gen.engine
    loss0, terms0 = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False)
    grads0 = gen.grad_bucket.flat.clone()
    assert gen.last_aux is None
    loss, terms = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False, aux=AuxLoss())
    assert _same_bits(loss, loss0) and _same_bits(terms, terms0) and _same_bits(gen.grad_bucket.flat, grads0)
    assert len(gen.last_aux) == 2 and "stoi_loss" not in eng._wss       # all weights 0: the bits and launches of today
    aux = AuxLoss(w_stoi=0.5, stoi_extended=extended)
    loss1, terms1 = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False, aux=aux)
    grads1 = gen.grad_bucket.flat.clone()
    total1, rows1, stoi_rows1 = (t.clone() for t in gen.last_aux)
    assert _same_bits(terms1, terms0) and not torch.equal(grads1, grads0) and tuple(rows1.shape) == (B, 0)
    # forward, Engine.stoi_loss, cmgan_loss_backward_aux, gen.backward
    c = eng.rms_scale(noisy)
    noisy_spec, clean_spec = eng.stft_compress(noisy, c), eng.stft_compress(clean, c)
    T = noisy_spec.shape[2]
    est_real, est_imag = gen.forward(noisy_spec, None)
    est_audio = eng.uncompress_istft(est_real, est_imag)
    clean_cut = clean[:, :est_audio.shape[-1]].contiguous()
    base, _ = generator_loss_terms(eng, est_real, est_imag, clean_spec, est_audio, clean_cut, w)
    out = eng.stoi_loss(est_audio, clean_cut * c[:, None], 0.5, extended)
    d_real, d_imag = torch.empty_like(est_real), torch.empty_like(est_imag)
    eng._call("cmgan_loss_backward_aux", est_real, est_imag, clean_spec, B, T, est_audio, clean_cut, *w, out.grad, d_real, d_imag)
    want_real, want_imag = d_real.clone(), d_imag.clone()
    gen.backward(d_real, d_imag)
    assert _same_bits(gen.grad_bucket.flat, grads1)
    assert _same_bits(out.rows, stoi_rows1) and _same_bits(out.total[0], total1[0]) and _same_bits(out.total[0], total1[3])
    assert float(total1[1]) == 0.0 and float(total1[2]) == 0.0
    assert _same_bits(base, loss0) and _same_bits(loss1, base + out.total[0])
    assert int(out.status[0]) == 0 and 0.0 < float(out.rows[0, 0]) < 1.0 and float(out.total[0]) < 0.0
    # d_real / d_imag of the step itself: the step's own backward input, recomputed through the step's helpers
    from cmgan_amd.training import _aux_term, _loss_backward
    aux_out = _aux_term(gen, aux, est_audio, clean_cut, c)
    got_real, got_imag = _loss_backward(eng, aux_out, est_real, est_imag, clean_spec, est_audio, clean_cut, w)
    assert _same_bits(got_real, want_real) and _same_bits(got_imag, want_imag)
    assert aux_out.grad.data_ptr() != est_audio.data_ptr()


def test_graphed_train_step_with_w_stoi_is_bit_identical_to_the_eager_step(clips):
    """Two eager steps made before the capture against two replays (the layout of the auxiliary losses' graphed test)."""
    from cmgan_amd.training import AuxLoss, GraphedTrainStep, generator_train_step
    clean, noisy = clips
    B, L = clean.shape
    aux = AuxLoss(w_stoi=0.5, stoi_extended=True)
    gen, og = _fresh()
    want = []
    for _ in range(2):
        out = generator_train_step(gen, og, clean, noisy, (0.1, 0.9, 0.2), masks=None, aux=aux)
        want.append([t.clone() for t in (*out, *gen.last_aux, gen.param_bucket.flat)])
    gen2, og2 = _fresh()
    step = GraphedTrainStep(gen2, og2, B, L, dropout=False, aux=aux)
    assert len(step.last_aux) == 3 and "aux_loss" not in gen2.engine._wss
    for i in range(2):
        got = (*step(clean, noisy), *step.last_aux, gen2.param_bucket.flat)
        assert all(_same_bits(x, y) for x, y in zip(want[i], got)), i
    assert not _same_bits(want[0][-2], want[1][-2])                     # the term's value moved with the parameters


def test_stoi_joins_the_other_auxiliary_terms_with_one_add(clips):
    from cmgan_amd.training import AuxLoss, _aux_term
    clean, noisy = clips
    gen, _ = _fresh()
    eng = gen.engine
    c = eng.rms_scale(noisy)
    est_audio = (0.8 * noisy * c[:, None]).contiguous()
    clean_cut = clean.contiguous()
    aux = AuxLoss((512, 1024), w_mr=1.0, w_si=0.05, w_stoi=0.5)
    got = _aux_term(gen, aux, est_audio, clean_cut, c)
    target = clean_cut * c[:, None]
    st = eng.stoi_loss(est_audio, target, 0.5, False)
    ax = eng.aux_loss(est_audio, target, (512, 1024), 1.0, 0.05)
    assert _same_bits(got.grad, ax.grad + st.grad) and _same_bits(got.total[0], ax.total[0] + st.total[0])
    assert _same_bits(got.total[1:3], ax.total[1:]) and _same_bits(got.total[3], st.total[0])
    total, rows, stoi_rows = gen.last_aux
    assert _same_bits(rows, ax.rows) and _same_bits(stoi_rows, st.rows) and _same_bits(total, got.total)
