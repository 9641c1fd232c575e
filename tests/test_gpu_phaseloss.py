"""GPU tests of the phase loss (cmgan_amd/csrc/phaseloss.hip: Engine.phase_loss, the `w_ip` / `w_gd` / `w_iaf` terms of
training.AuxLoss) against the numpy model of tests/phaseloss_model.py, whose docstring states the acceptance rule, the values'
bound and the two margins; tests/test_phaseloss_host.py checks, without a GPU, that every case meets them.  No sample is
left out of any comparison.

Shapes (phaseloss_model.SHAPES): F = 201 at T = 1, 2, 3 and T = 17 - the kernels cut a row into tiles of 8 frames, so 17 is
two whole tiles and one of a single frame: pairs cross a tile edge twice, and the last tile is one frame and its halo - and
F = 601 at T = 2: a thread of the 256 walks bins f, f + 256, f + 512, so 601 is two whole passes and a part of a third (201 is
less than one).  Batches of three rows (phaseloss_model.BATCHES): `main` = a random estimate against a random clean row, a
row with exact-zero cells in both spectra at the corners, inside and next to each other, est == clean bit for bit; `odd` =
est = 2 clean, a row with a NaN and two infinities, a row whose estimate is all zeros; `floor` = two rows with a tenth of each
spectrum below the floor of 1e-2 around a random one, called with that floor; `lone` = the random row alone (B = 1).

Measured on an MI355X over every judged row: counts and status words equal; the worst value error is 4.0e-16 = 1.144 u pi (the
row with the NaN at T = 17; bounds 7.9e-15 .. 1.3e-14, of which the atan2 allowance is 4.6 u pi); no gradient sample lies beyond
half an ulp of the long-double value (excess 0 of E on every row)."""
import numpy as np
import pytest
import torch

import phaseloss_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = M.K_WEIGHTS
TILES = (17, 201)                   # the shape with three tiles


@pytest.fixture(scope="module")
def engines():
    """An Engine per F: 201 bins are n_fft 400 / hop 100, 601 bins n_fft 1200 / hop 300."""
    from cmgan_amd.engine import Engine
    return {201: Engine(device=DEV), 601: Engine(n_fft=1200, hop=300, device=DEV)}


@pytest.fixture(scope="module")
def eng(engines):
    return engines[201]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_same(x, y):
    return all((p is None and q is None) or _same_bits(p, q) for p, q in zip(x, y))


def _judge(out, kinds, nT, nF, weights, floor, tag):
    """Every output of one call against the model: counts and status for equality, values inside their bound, every
    gradient sample by the acceptance rule, the total inside what its rows allow."""
    B = len(kinds)
    k3 = tuple(w / B for w in weights)
    assert out.rows.dtype == torch.float64 and tuple(out.rows.shape) == (B, 3)
    assert out.counts.dtype == torch.int32 and tuple(out.counts.shape) == (B, 3)
    assert out.status.dtype == torch.int32 and tuple(out.status.shape) == (B,)
    assert out.total.dtype == torch.float32 and tuple(out.total.shape) == (4,)
    assert tuple(out.g_real.shape) == tuple(out.g_imag.shape) == (B, 1, nT, nF)
    rows, counts, status = out.rows.cpu().numpy(), out.counts.cpu().numpy(), out.status.cpu().numpy()
    g_real, g_imag = out.g_real.cpu().numpy()[:, 0], out.g_imag.cpu().numpy()[:, 0]
    bound = M.value_bound(nT, nF)
    want, slack = np.zeros(4, dtype=M.LD), 0.0
    for b, kind in enumerate(kinds):
        m = M.row_model(kind, nT, nF, k3, floor)
        assert m.branch_margin >= M.BRANCH_MARGIN and m.floor_margin >= M.FLOOR_MARGIN, (kind, m.branch_margin, m.floor_margin)
        assert list(counts[b]) == list(m.counts) and int(status[b]) == m.status, (tag, kind, counts[b], status[b], m.counts, m.status)
        err = float(np.max(np.abs(rows[b].astype(M.LD) - m.values)))
        ok, frac = M.accept(g_real[b], g_imag[b], m)
        print(f"[phaseloss] {tag} T={nT} F={nF} row {kind}: value error = {err:.2e} = {err / (M.U * np.pi):.3f} u pi (bound {bound:.2e}), "
              f"gradient excess = {frac:.3f} of E")
        assert err <= bound and err <= M.VALUE_CAP, (tag, kind, err, bound)
        assert ok, (tag, kind, frac)
        if kind in ("same", "double", "void"):
            assert not rows[b].any(), (kind, rows[b])                   # exact zeros
        if kind in ("same", "void"):
            assert not g_real[b].any() and not g_imag[b].any(), kind
        for i in range(3):                                              # a count of 0: value 0
            assert counts[b, i] > 0 or rows[b, i] == 0.0
        want += np.array([m.a, *m.parts], dtype=M.LD)
        slack += sum(k3) * bound
    got = out.total.cpu().numpy().astype(np.float64)
    for i in range(4):
        assert abs(M.LD(got[i]) - want[i]) <= M.ulp32(float(want[i])) / 2 + slack + 8 * M.U * abs(float(want[i])), (tag, i, got, want)


# ------------------------------------------------------------------ values and gradients
@pytest.mark.parametrize("name", ["main", "odd", "floor", "lone"])
@pytest.mark.parametrize("nT,nF", M.SHAPES)
def test_values_and_gradients_against_the_model(engines, nT, nF, name):
    eng = engines[nF]
    est_real, est_imag, clean, kinds, floor = M.batch(name, nT, nF)
    out = eng.phase_loss(*_dev(est_real, est_imag, clean), *W, floor)
    _judge(out, kinds, nT, nF, W, floor, name)
    status = out.status.cpu().numpy()
    for b, kind in enumerate(kinds):
        assert int(status[b]) == (7 if kind == "void" else (4 if nT == 1 else 0)), (kind, status[b])


def test_the_void_rule_at_and_around_the_zero_cells(eng):
    """The gradient at a void cell is an exact zero; around it, the terms that touch the cell are gone: the samples there are
    the model's, which differ from the ones the same row has without the zero cells."""
    nT, nF = TILES
    est_real, est_imag, clean, kinds, floor = M.batch("main", nT, nF)
    b = kinds.index("zeros")
    out = eng.phase_loss(*_dev(est_real, est_imag, clean), *W, floor)
    ze, zc = M.zero_cells(nT, nF)
    g_real, g_imag = out.g_real.cpu().numpy()[b, 0], out.g_imag.cpu().numpy()[b, 0]
    counts = out.counts.cpu().numpy()[b]
    void = np.zeros((nT, nF), dtype=bool)
    for t, f in ze + zc:
        void[t, f] = True
        assert g_real[t, f] == 0.0 and g_imag[t, f] == 0.0 and not np.signbit(g_real[t, f]) and not np.signbit(g_imag[t, f])
    ok = ~void
    assert list(counts) == [int(ok.sum()), int((ok[:, 1:] & ok[:, :-1]).sum()), int((ok[1:] & ok[:-1]).sum())]
    # the neighbours of (tm, fm), an interior void cell of the estimate: judged sample by sample above; here, that they moved
    filled = [x.copy() for x in (est_real, est_imag, clean)]
    t, f = nT // 2, nF // 2
    filled[0][b, 0, t, f] = filled[1][b, 0, t, f] = 0.25
    full = eng.phase_loss(*_dev(*filled), *W, floor)
    assert int(full.counts[b, 0]) == counts[0] + 1
    for dt, df in ((0, -1), (-1, 0), (1, 0)):
        assert float(full.g_real[b, 0, t + dt, f + df]) != float(g_real[t + dt, f + df])


@pytest.mark.parametrize("zero", [(0,), (1,), (2,), (0, 2), (0, 1, 2)], ids=["ip", "gd", "iaf", "ip+iaf", "all"])
def test_a_weight_of_zero_leaves_its_term_out(eng, zero):
    nT, nF = TILES
    est_real, est_imag, clean, kinds, floor = M.batch("main", nT, nF)
    w = tuple(0.0 if i in zero else W[i] for i in range(3))
    out = eng.phase_loss(*_dev(est_real, est_imag, clean), *w, floor)
    _judge(out, kinds, nT, nF, w, floor, "k=0")
    ref = eng.phase_loss(*_dev(est_real, est_imag, clean), *W, floor)
    assert _same_bits(out.rows, ref.rows) and _same_bits(out.counts, ref.counts) and _same_bits(out.status, ref.status)
    for i in zero:
        assert float(out.total[1 + i]) == 0.0
    if len(zero) == 3:
        assert not bool(out.g_real.any()) and not bool(out.g_imag.any()) and float(out.total[0]) == 0.0
    else:
        assert not _same_bits(out.g_real, ref.g_real)


# ------------------------------------------------------------------ reproducibility, independence, capture
def test_reproducible_values_alone_not_in_place_and_capturable(eng):
    nT, nF = TILES
    est_real, est_imag, clean, kinds, floor = M.batch("main", nT, nF)
    er, ei, cs = _dev(est_real, est_imag, clean)
    a = eng.phase_loss(er, ei, cs, *W, floor)
    b = eng.phase_loss(er, ei, cs, *W, floor)
    assert _all_same(a, b)
    s = eng.phase_loss(er, ei, cs, *W, floor, grad=False)
    assert s.g_real is None and s.g_imag is None and _all_same(s[:4], a[:4])
    # the gradient is never formed over an input, nor the two halves over each other: refused before anything is launched
    B = len(kinds)
    ws = eng._wss["phase_loss"]
    rows, counts = torch.full_like(a.rows, 7.0), torch.full_like(a.counts, 7)
    total, status = torch.full_like(a.total, 7.0), torch.full_like(a.status, 7)
    g1, g2 = torch.full_like(er, 7.0), torch.full_like(er, 7.0)
    keep = [t.clone() for t in (er, ei, cs)]
    for gr, gi, text in ((er, g2, b"overlaps an input"), (g1, ei, b"overlaps an input"), (cs[:, 1:], g2, b"overlaps an input"),
                         (g1, cs[:, :1], b"overlaps an input"), (g1, g1, b"g_real overlaps g_imag")):
        rc = eng.lib.cmgan_phase_loss(eng._h, er.data_ptr(), ei.data_ptr(), cs.data_ptr(), B, nT, 0.1, 0.1, 0.1, 0.0,
                                      rows.data_ptr(), counts.data_ptr(), total.data_ptr(), status.data_ptr(), gr.data_ptr(),
                                      gi.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream())
        torch.cuda.synchronize()
        assert rc == -1 and text in eng.lib.cmgan_last_error(eng._h), (rc, eng.lib.cmgan_last_error(eng._h))
    assert all(torch.equal(x, y) for x, y in zip(keep, (er, ei, cs)))
    assert all(bool((t == 7).all()) for t in (rows, counts, total, status, g1, g2))
    # captured and replayed on new contents of the static inputs (other void cells and counts than at the capture)
    ser, sei, scs = torch.ones_like(er), torch.ones_like(ei).mul_(-0.5), torch.ones_like(cs)
    ser[:, :, ::2, ::3] = 0.0
    sei[:, :, ::2, ::3] = 0.0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = eng.phase_loss(ser, sei, scs, *W, floor)
    ser.copy_(er)
    sei.copy_(ei)
    scs.copy_(cs)
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(got[1:], a[1:]) and _same_bits(got.total, a.total)


@pytest.mark.parametrize("nT,nF", [TILES, (2, 601)])
def test_a_row_has_the_bits_it_has_alone_and_beside_other_neighbours(engines, nT, nF):
    eng = engines[nF]
    est_real, est_imag, clean, kinds, floor = M.batch("main", nT, nF)
    er, ei, cs = _dev(est_real, est_imag, clean)
    out = eng.phase_loss(er, ei, cs, *W, floor)
    B = len(kinds)
    ia = kinds.index("rand")

    def row_of(o, b):
        return o.rows[b], o.counts[b], o.status[b:b + 1], o.g_real[b], o.g_imag[b]
    one = eng.phase_loss(er[ia:ia + 1].contiguous(), ei[ia:ia + 1].contiguous(), cs[ia:ia + 1].contiguous(), *(w / B for w in W),
                         floor)                                          # the same k
    assert _all_same(row_of(one, 0), row_of(out, ia))
    order = [2, 0, 1]                                                   # other neighbours, another place in the batch
    mixed = eng.phase_loss(er[order].contiguous(), ei[order].contiguous(), cs[order].contiguous(), *W, floor)
    for new, old in enumerate(order):
        assert _all_same(row_of(mixed, new), row_of(out, old)), (new, old)
    # a NaN beside it stays in its own row, where it voids its cell and nothing else
    e2, c2 = er.clone(), cs.clone()
    e2[1, 0, nT - 1, 9] = float("nan")
    c2[2, 1, 0, 3] = float("inf")
    bad = eng.phase_loss(e2, ei, c2, *W, floor)
    assert _all_same(row_of(bad, ia), row_of(out, ia)) and bool(torch.isfinite(bad.total).all()) and bool(torch.isfinite(bad.rows).all())
    assert int(bad.counts[1, 0]) == int(out.counts[1, 0]) - 1 and int(bad.counts[2, 0]) == int(out.counts[2, 0]) - 1
    assert float(bad.g_real[1, 0, nT - 1, 9]) == 0.0 and float(bad.g_imag[2, 0, 0, 3]) == 0.0
    assert bool(torch.isfinite(bad.g_real).all()) and bool(torch.isfinite(bad.g_imag).all())


# ------------------------------------------------------------------ wiring into the training step
TRAIN_B, TRAIN_L = 2, 3200          # the 2 x 33 frames tests/test_gpu_training.py steps at
W3 = (0.1, 0.9, 0.2)


@pytest.fixture(scope="module")
def clips():
    from cmgan_amd.synth import synthetic_clips
    clean = synthetic_clips(TRAIN_B, TRAIN_L, seed=5).to(DEV)
    noisy = (clean + 0.3 * synthetic_clips(TRAIN_B, TRAIN_L, seed=6).to(DEV)).contiguous()
    return clean, noisy


def _fresh():
    from cmgan_amd.training import AdamW, GeneratorTrain
    from oracle.weights import make_state_dict
    gen = GeneratorTrain(make_state_dict(seed=0), device=DEV)
    return gen, AdamW(gen.engine, gen.param_bucket, gen.grad_bucket, lr=5e-4)


def _phase_only():
    from cmgan_amd.training import AuxLoss
    return AuxLoss(w_ip=0.3, w_gd=0.2, w_iaf=0.1, phase_floor=1e-3)


def _with_si():
    from cmgan_amd.training import AuxLoss
    return AuxLoss(w_si=0.05, w_ip=0.3, w_gd=0.2, w_iaf=0.1, phase_floor=1e-3)


@pytest.mark.parametrize("make", [_phase_only, _with_si], ids=["phase", "phase+si"])
def test_generator_train_step_with_phase_weights_is_the_manual_composition(clips, make):
    from cmgan_amd.training import generator_loss_terms, generator_train_step
    clean, noisy = clips
    B = clean.shape[0]
    aux = make()
    gen, opt = _fresh()
    eng = gen.engine
    loss0, terms0 = generator_train_step(gen, opt, clean, noisy, W3, masks=None, update=False)
    grads0 = gen.grad_bucket.flat.clone()
    assert gen.last_phase is None and "phase_loss" not in eng._wss
    loss1, terms1 = generator_train_step(gen, opt, clean, noisy, W3, masks=None, update=False, aux=aux)
    grads1 = gen.grad_bucket.flat.clone()
    last = tuple(t.clone() for t in gen.last_phase)
    assert len(last) == 4 and _same_bits(terms1, terms0) and not torch.equal(grads1, grads0)
    if aux.w_si == 0.0:                                                 # phase alone: no audio-domain term is run at all
        assert gen.last_aux is None and "aux_loss" not in eng._wss and "stoi_loss" not in eng._wss
    else:
        assert len(gen.last_aux) == 2 and tuple(gen.last_aux[0].shape) == (3,) and "stoi_loss" not in eng._wss
    # forward, Engine.phase_loss, cmgan_loss_backward (or _aux), one tensor add each, gen.backward
    c = eng.rms_scale(noisy)
    noisy_spec, clean_spec = eng.stft_compress(noisy, c), eng.stft_compress(clean, c)
    T = noisy_spec.shape[2]
    est_real, est_imag = gen.forward(noisy_spec, None)
    est_audio = eng.uncompress_istft(est_real, est_imag)
    clean_cut = clean[:, :est_audio.shape[-1]].contiguous()
    base, _ = generator_loss_terms(eng, est_real, est_imag, clean_spec, est_audio, clean_cut, W3)
    assert _same_bits(base, loss0)
    want_loss = base
    d_real, d_imag = torch.empty_like(est_real), torch.empty_like(est_imag)
    if aux.w_si == 0.0:
        eng._call("cmgan_loss_backward", est_real, est_imag, clean_spec, B, T, est_audio, clean_cut, *W3, d_real, d_imag)
    else:
        ax = eng.aux_loss(est_audio, clean_cut * c[:, None], aux.n_ffts, aux.w_mr, aux.w_si)
        want_loss = want_loss + ax.total[0]
        eng._call("cmgan_loss_backward_aux", est_real, est_imag, clean_spec, B, T, est_audio, clean_cut, *W3, ax.grad, d_real, d_imag)
        assert _same_bits(ax.total, gen.last_aux[0]) and _same_bits(ax.rows, gen.last_aux[1])
    ph = eng.phase_loss(est_real, est_imag, clean_spec, aux.w_ip, aux.w_gd, aux.w_iaf, aux.phase_floor)
    assert _all_same((ph.total, ph.rows, ph.counts, ph.status), last)
    assert _same_bits(loss1, want_loss + ph.total[0]) and float(ph.total[0]) > 0.0 and not bool(ph.status.any())
    d_real.add_(ph.g_real)
    d_imag.add_(ph.g_imag)
    gen.backward(d_real, d_imag)
    assert _same_bits(gen.grad_bucket.flat, grads1)
    assert ph.g_real.data_ptr() != est_real.data_ptr() and ph.g_imag.data_ptr() != est_imag.data_ptr()


@pytest.mark.parametrize("make", [_phase_only, _with_si], ids=["phase", "phase+si"])
def test_graphed_train_step_with_phase_weights_is_bit_identical_to_the_eager_step(clips, make):
    """Two eager steps made before the capture against two replays (the layout of the auxiliary losses' graphed test)."""
    from cmgan_amd.training import GraphedTrainStep, generator_train_step
    clean, noisy = clips
    B, L = clean.shape
    aux = make()
    gen, og = _fresh()
    want = []
    for _ in range(2):
        out = generator_train_step(gen, og, clean, noisy, W3, masks=None, aux=aux)
        want.append([t.clone() for t in (*out, *gen.last_phase, *(gen.last_aux or ()), gen.param_bucket.flat)])
    gen2, og2 = _fresh()
    step = GraphedTrainStep(gen2, og2, B, L, dropout=False, aux=aux)
    assert len(step.last_phase) == 4 and (step.last_aux is None) == (aux.w_si == 0.0)
    assert ("aux_loss" in gen2.engine._wss) == (aux.w_si != 0.0) and "phase_loss" in gen2.engine._wss
    for i in range(2):
        got = (*step(clean, noisy), *step.last_phase, *(step.last_aux or ()), gen2.param_bucket.flat)
        assert len(got) == len(want[i]) and all(_same_bits(x, y) for x, y in zip(want[i], got)), i
    assert not _same_bits(want[0][3], want[1][3])                       # the term's rows moved with the parameters


def test_phase_weights_of_zero_are_the_step_without_the_fields(clips):
    from cmgan_amd.training import AuxLoss, generator_train_step
    clean, noisy = clips
    gen, opt = _fresh()
    eng = gen.engine
    results = []
    for aux in (AuxLoss(w_si=0.05), AuxLoss(w_si=0.05, w_ip=0.0, w_gd=0.0, w_iaf=0.0, phase_floor=0.25), AuxLoss(), AuxLoss(phase_floor=1.0)):
        loss, terms = generator_train_step(gen, opt, clean, noisy, W3, masks=None, update=False, aux=aux)
        assert gen.last_phase is None and "phase_loss" not in eng._wss and len(gen.last_aux) == 2
        results.append((loss.clone(), terms.clone(), gen.grad_bucket.flat.clone(), *(t.clone() for t in gen.last_aux)))
    assert _all_same(results[0], results[1]) and _all_same(results[2], results[3])
    assert not _same_bits(results[0][2], results[2][2])


def test_the_adversarial_half_adds_the_phase_gradient_before_the_gan_term_joins(clips):
    from cmgan_amd.synth import discriminator_state_dict
    from cmgan_amd.training import DiscriminatorTrain, _adversarial_generator_half, generator_loss_terms
    clean, noisy = clips
    B = clean.shape[0]
    w4 = (*W3, 0.05)
    aux = _phase_only()
    gen, _ = _fresh()
    disc = DiscriminatorTrain(discriminator_state_dict(0), engine=gen.engine)
    loss, terms, gan, _ = _adversarial_generator_half(gen, disc, clean, noisy, w4, None, None, None, aux)
    grads = gen.grad_bucket.flat.clone()
    last = tuple(t.clone() for t in gen.last_phase)
    assert gen.last_aux is None
    gen2, _ = _fresh()
    eng = gen2.engine
    disc2 = DiscriminatorTrain(discriminator_state_dict(0), engine=eng)
    c = eng.rms_scale(noisy)
    noisy_spec, clean_spec = eng.stft_compress(noisy, c), eng.stft_compress(clean, c)
    T = noisy_spec.shape[2]
    est_real, est_imag = gen2.forward(noisy_spec, None)
    est_audio = eng.uncompress_istft(est_real, est_imag)
    clean_cut = clean[:, :est_audio.shape[-1]].contiguous()
    base, _ = generator_loss_terms(eng, est_real, est_imag, clean_spec, est_audio, clean_cut, W3)
    xy = disc2.pair(clean_spec, est_real, est_imag)
    gan2, dscore = disc2.score_mse(disc2.forward(xy, None, train=True, slot=0), None, scale=w4[3])
    ph = eng.phase_loss(est_real, est_imag, clean_spec, aux.w_ip, aux.w_gd, aux.w_iaf, aux.phase_floor)
    d_real, d_imag = torch.empty_like(est_real), torch.empty_like(est_imag)
    eng._call("cmgan_loss_backward", est_real, est_imag, clean_spec, B, T, est_audio, clean_cut, *W3, d_real, d_imag)
    d_real.add_(ph.g_real)
    d_imag.add_(ph.g_imag)
    dxy = disc2.backward(dscore, slot=0, need_input_grad=True)
    eng._call("cmgan_mag_pair_backward", est_real, est_imag, dxy, B, T, 1.0, d_real, d_imag)
    gen2.backward(d_real, d_imag)
    assert _same_bits(gan, gan2) and _same_bits(loss, (base + w4[3] * gan2) + ph.total[0])
    assert _all_same((ph.total, ph.rows, ph.counts, ph.status), last) and _same_bits(gen2.grad_bucket.flat, grads)
