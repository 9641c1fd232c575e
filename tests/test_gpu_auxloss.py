"""GPU tests of the auxiliary losses (cmgan_amd/csrc/auxloss.hip: Engine.aux_loss; cmgan_loss_backward_aux; the `aux=` option
of the training entry points) against the numpy model of tests/auxloss_model.py, whose docstring states the acceptance
rule.  Smallest shapes that reach every edge: L = 1100 (three frames of the 2048 window, both margins fold onto most of the
row), 1700 (a multiple of no hop), 3200; one to four resolutions.

Measured on an MI355X over every judged row: no gradient sample lies beyond half an ulp of the long-double value (the worst
excess is 0 of E); the worst `rows` error is 0.006 of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import auxloss_model as M
from conftest import rel_err
from oracle import cmgan_oracle as O
from test_gpu_training import GRAD_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL = (256, 512, 1024, 2048)


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _judge(out, keys, n_ffts, w_mr, w_si, what):
    """rows, total and (when there is one) the gradient of `out` against the model of the rows `keys`."""
    B = len(keys)
    k_mr, k_si = w_mr / B, w_si / B
    models = [M.row_model(k, n_ffts, k_mr, k_si) for k in keys]
    rows = out.rows.cpu().numpy()
    worst_v = worst_g = 0.0
    for b, m in enumerate(models):
        err = np.abs(rows[b].astype(M.LD) - m.rows).astype(np.float64)
        worst_v = max(worst_v, float(np.max(err / m.bounds)))
        if out.grad is not None:
            ok, frac = M.accept(out.grad[b].cpu().numpy(), m)
            worst_g = max(worst_g, frac)
            assert ok, (what, b, frac, m.E)
    print(f"[auxloss] {what}: worst rows error = {worst_v:.3f} of its bound, worst gradient excess = {worst_g:.3f} of E")
    assert worst_v <= 1.0, (what, worst_v)
    R = len(n_ffts)
    slack = sum(k_mr * float(np.sum(m.bounds[:-1])) / R + k_si * float(m.bounds[-1]) for m in models)
    for i, part in enumerate(("a", "a_mr", "a_si")):
        want = sum((getattr(m, part) for m in models), M.LD(0))
        got = float(out.total[i])
        assert abs(M.LD(got) - want) <= M.ulp32(float(want)) / 2 + slack + 8 * M.U * abs(float(want)), (what, part, got, float(want))


# ------------------------------------------------------------------ values and gradients
@pytest.mark.parametrize("n_ffts", M.N_FFT_SETS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("L", M.LENGTHS)
def test_values_and_gradients_against_the_model(eng, L, n_ffts):
    est, ref = _dev(*M.batch(L))
    keys = [M.registered(L, b) for b in range(M.B)]
    for w_mr, w_si in M.WEIGHTS:
        out = eng.aux_loss(est, ref, n_ffts, w_mr, w_si)
        assert out.rows.dtype == torch.float64 and tuple(out.rows.shape) == (M.B, 2 * len(n_ffts) + 1)
        assert out.total.dtype == torch.float32 and out.grad.dtype == torch.float32 and tuple(out.grad.shape) == (M.B, L)
        _judge(out, keys, n_ffts, w_mr, w_si, f"L={L} n_ffts={n_ffts} w=({w_mr}, {w_si})")


@pytest.mark.parametrize("L", M.LENGTHS)
def test_identical_row_is_exactly_zero(eng, L):
    est, ref = M.batch(L)
    est = est.copy()
    est[1] = ref[1]
    est, ref = _dev(est, ref)
    for n_ffts in M.N_FFT_SETS:
        out = eng.aux_loss(est, ref, n_ffts, 1.0, 0.0)
        assert torch.all(out.rows[1, :-1] == 0), (n_ffts, out.rows[1])
        assert torch.all(out.grad[1] == 0), n_ffts
        assert torch.all(out.rows[0, :-1] > 0) and bool(out.grad[0].abs().max() > 0) and bool(torch.isfinite(out.rows).all())


@pytest.mark.parametrize("L", M.LENGTHS)
def test_all_zero_estimate_row(eng, L):
    est, ref = M.batch(L)
    est = est.copy()
    est[2] = 0.0
    keys = [M.registered(L, 0), M.registered(L, 1), M.register(("zero", L, 2), est[2], ref[2])]
    est, ref = _dev(est, ref)
    for w_mr, w_si in M.WEIGHTS:
        out = eng.aux_loss(est, ref, FULL, w_mr, w_si)
        assert torch.all(out.grad[2] == 0), (w_mr, w_si)
        assert float(out.rows[2, -1]) == 0.0                            # S = Q = 1e-8
        _judge(out, keys, FULL, w_mr, w_si, f"zero estimate row, L={L} w=({w_mr}, {w_si})")


# ------------------------------------------------------------------ row independence, reproducibility, capture
def test_a_row_has_the_bits_it_has_alone_and_keeps_them_beside_a_nan(eng):
    L = 1700
    est, ref = _dev(*M.batch(L))
    w_mr, w_si = M.W_MR, M.W_SI
    out = eng.aux_loss(est, ref, FULL, w_mr, w_si)
    for b in range(M.B):
        one = eng.aux_loss(est[b:b + 1].contiguous(), ref[b:b + 1].contiguous(), FULL, w_mr / M.B, w_si / M.B)
        assert _same_bits(one.rows[0], out.rows[b]) and _same_bits(one.grad[0], out.grad[b]), b
    for where in ("est", "ref"):
        e2, r2 = est.clone(), ref.clone()
        (e2 if where == "est" else r2)[1, 777] = float("nan")
        bad = eng.aux_loss(e2, r2, FULL, w_mr, w_si)
        for b in (0, 2):
            assert _same_bits(bad.rows[b], out.rows[b]) and _same_bits(bad.grad[b], out.grad[b]), (where, b)
        assert not bool(torch.isfinite(bad.rows[1]).all()) and not bool(torch.isfinite(bad.total[0]))
        assert not bool(torch.isfinite(bad.grad[1]).all())


def test_reproducible_scorer_not_in_place_and_capturable(eng):
    L = 1700
    est, ref = _dev(*M.batch(L))
    w_mr, w_si = M.W_MR, M.W_SI
    a = eng.aux_loss(est, ref, FULL, w_mr, w_si)
    b = eng.aux_loss(est, ref, FULL, w_mr, w_si)
    assert all(_same_bits(x, y) for x, y in zip(a, b))
    s = eng.aux_loss(est, ref, FULL, w_mr, w_si, grad=False)
    assert s.grad is None and _same_bits(s.rows, a.rows) and _same_bits(s.total, a.total)
    # the gradient is never formed in place: refused before anything is launched
    scratch = est.clone()
    ws = eng._aux_workspace(M.B, L, FULL)
    arr = (ctypes.c_int * 4)(*FULL)
    rows, total = torch.full_like(a.rows, 7.0), torch.full_like(a.total, 7.0)
    rc = eng.lib.cmgan_aux_loss(eng._h, scratch.data_ptr(), ref.data_ptr(), M.B, L, 4, arr, w_mr / M.B, w_si / M.B, rows.data_ptr(),
                                total.data_ptr(), scratch.data_ptr(), ws.data_ptr(), ws.numel(), eng._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"g_audio overlaps" in eng.lib.cmgan_last_error(eng._h)
    assert torch.equal(scratch, est) and bool((rows == 7.0).all()) and bool((total == 7.0).all())
    # captured and replayed on new contents of the static inputs
    se, sr = torch.ones_like(est), torch.ones_like(ref).mul_(0.5)
    se[:, ::2] = -1.0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = eng.aux_loss(se, sr, FULL, w_mr, w_si)
    se.copy_(est)
    sr.copy_(ref)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(got, a))


# ------------------------------------------------------------------ the loss backward with a waveform gradient
@pytest.mark.parametrize("T", [9, 17])
def test_loss_backward_aux(eng, T):
    B, F = 2, 201
    rng = np.random.Generator(np.random.PCG64(400 + T))
    er, ei, cr = (torch.from_numpy((0.5 * rng.standard_normal(s)).astype(np.float32)) for s in ((B, 1, T, F), (B, 1, T, F), (B, 2, T, F)))
    La = 100 * (T - 1)
    clean = torch.from_numpy((0.1 * rng.standard_normal((B, La))).astype(np.float32))
    g_audio = torch.from_numpy((1e-3 * rng.standard_normal((B, La))).astype(np.float32))
    der, dei, dcs, dclean, dg = (t.to(DEV).contiguous() for t in (er, ei, cr, clean, g_audio))
    audio = eng.uncompress_istft(der, dei)

    def run(name, w, a, c, g=None):
        d_real, d_imag = torch.full_like(der, 7.0), torch.full_like(dei, 7.0)
        args = [der, dei, dcs, B, T, a, c, *w] + ([g] if name.endswith("_aux") else []) + [d_real, d_imag]
        eng._call(name, *args)
        return d_real, d_imag

    for w, a, c in (((0.1, 0.9, 0.2), audio, dclean), ((0.3, 0.7, 0.0), None, None), ((0.3, 0.7, 0.0), audio, dclean)):
        want = run("cmgan_loss_backward", w, a, c)
        got = run("cmgan_loss_backward_aux", w, a, c, None)
        assert _same_bits(want[0], got[0]) and _same_bits(want[1], got[1]), w
    for w, nullaudio in (((0.1, 0.9, 0.2), False), ((0.3, 0.7, 0.0), True), ((0.3, 0.7, 0.0), False)):
        erl, eil = er.double().requires_grad_(True), ei.double().requires_grad_(True)
        with torch.enable_grad():
            est_audio = O.uncompress_istft(erl, eil)
            out = {"est_real": erl, "est_imag": eil, "clean_spec": cr.double(), "est_audio": est_audio}
            loss = O.generator_loss(out, clean.double(), w)[0] + (g_audio.double() * est_audio).sum()
            loss.backward()
        got = run("cmgan_loss_backward_aux", w, None if nullaudio else audio, None if nullaudio else dclean, dg)
        e_r, e_i = rel_err(got[0], erl.grad.float()), rel_err(got[1], eil.grad.float())
        print(f"[parity] loss backward aux T={T} w={w} null audio={nullaudio}: rel_err = {e_r:.3e}, {e_i:.3e}")
        assert e_r < GRAD_TOL and e_i < GRAD_TOL
        plain = run("cmgan_loss_backward", w, None if nullaudio else audio, None if nullaudio else dclean)
        assert not torch.equal(plain[0], got[0])
    with pytest.raises(Exception, match="needs est_audio and clean_audio"):
        run("cmgan_loss_backward_aux", (0.1, 0.9, 0.2), None, None, dg)


# ------------------------------------------------------------------ wiring into the training steps
@pytest.fixture(scope="module")
def clips():
    from cmgan_amd.synth import synthetic_clips
    B, L = 2, 3200
    clean = synthetic_clips(B, L, seed=5).to(DEV)
    noisy = (clean + 0.3 * synthetic_clips(B, L, seed=6).to(DEV)).contiguous()
    return clean, noisy


def _fresh():
    from cmgan_amd.training import AdamW, GeneratorTrain
    from oracle.weights import make_state_dict
    gen = GeneratorTrain(make_state_dict(seed=0), device=DEV)
    return gen, AdamW(gen.engine, gen.param_bucket, gen.grad_bucket, lr=5e-4)


def test_generator_train_step_with_aux_is_the_manual_composition(clips):
    from cmgan_amd.training import AuxLoss, generator_loss_terms, generator_train_step
    clean, noisy = clips
    B = clean.shape[0]
    w = (0.1, 0.9, 0.2)
    gen, opt = _fresh()
    eng = gen.engine
    loss0, terms0 = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False)
    grads0 = gen.grad_bucket.flat.clone()
    assert gen.last_aux is None
    for off in (None, AuxLoss(), AuxLoss((256,), 0.0, 0.0)):
        loss, terms = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False, aux=off)
        assert _same_bits(loss, loss0) and _same_bits(terms, terms0) and _same_bits(gen.grad_bucket.flat, grads0), off
    aux = AuxLoss((512, 1024, 2048), w_mr=1.0, w_si=0.05)
    loss1, terms1 = generator_train_step(gen, opt, clean, noisy, w, masks=None, update=False, aux=aux)
    grads1 = gen.grad_bucket.flat.clone()
    total1, rows1 = (t.clone() for t in gen.last_aux)
    assert tuple(terms1.shape) == (4,) and _same_bits(terms1, terms0) and not torch.equal(grads1, grads0)
    # forward, Engine.aux_loss, cmgan_loss_backward_aux, gen.backward
    c = eng.rms_scale(noisy)
    noisy_spec, clean_spec = eng.stft_compress(noisy, c), eng.stft_compress(clean, c)
    T = noisy_spec.shape[2]
    est_real, est_imag = gen.forward(noisy_spec, None)
    est_audio = eng.uncompress_istft(est_real, est_imag)
    clean_cut = clean[:, :est_audio.shape[-1]].contiguous()
    base, _ = generator_loss_terms(eng, est_real, est_imag, clean_spec, est_audio, clean_cut, w)
    out = eng.aux_loss(est_audio, clean_cut * c[:, None], aux.n_ffts, aux.w_mr, aux.w_si)
    d_real, d_imag = torch.empty_like(est_real), torch.empty_like(est_imag)
    eng._call("cmgan_loss_backward_aux", est_real, est_imag, clean_spec, B, T, est_audio, clean_cut, *w, out.grad, d_real, d_imag)
    gen.backward(d_real, d_imag)
    assert _same_bits(gen.grad_bucket.flat, grads1)
    assert _same_bits(out.total, total1) and _same_bits(out.rows, rows1)
    assert _same_bits(base, loss0) and _same_bits(loss1, base + out.total[0])
    assert bool(torch.isfinite(out.rows).all()) and float(out.total[0]) > 0.0


@pytest.mark.parametrize("adversarial", [False, True])
def test_graphed_train_step_with_aux_is_bit_identical_to_the_eager_step(clips, adversarial):
    """The step with the auxiliary term, captured (its launches are part of the generator graph) and replayed three times,
    against three eager steps made before the capture: the layout of
    test_graphed_train_step_is_bit_identical_to_the_eager_step."""
    from cmgan_amd.synth import discriminator_state_dict
    from cmgan_amd.training import (AdamW, AuxLoss, DiscriminatorTrain, GraphedTrainStep, adversarial_train_step,
                                    generator_train_step)
    clean, noisy = clips
    B, L = clean.shape
    pesq = torch.tensor([0.4, 0.7], device=DEV)
    aux = AuxLoss((512, 1024, 2048), w_mr=1.0, w_si=0.05)

    def fresh():
        gen, og = _fresh()
        if not adversarial:
            return gen, None, og, None
        disc = DiscriminatorTrain(discriminator_state_dict(0), engine=gen.engine)
        return gen, disc, og, AdamW(gen.engine, disc.param_bucket, disc.grad_bucket, lr=1e-3)
    gen, disc, og, od = fresh()
    want = []
    for _ in range(3):
        if adversarial:
            out = adversarial_train_step(gen, disc, og, od, clean, noisy, pesq, masks=None, disc_masks=None, aux=aux)
            out = (out[0], out[1], out[3])
        else:
            out = generator_train_step(gen, og, clean, noisy, (0.1, 0.9, 0.2), masks=None, aux=aux)
        want.append([t.clone() for t in (*out, *gen.last_aux, gen.param_bucket.flat)])
    gen2, disc2, og2, od2 = fresh()
    step = GraphedTrainStep(gen2, og2, B, L, disc2, od2, dropout=False, aux=aux)
    assert og2.t == 0 and step.last_aux is not None
    for i in range(3):
        out = step(clean, noisy, pesq) if adversarial else step(clean, noisy)
        out = (out[0], out[1], out[3]) if adversarial else out
        got = (*out, *step.last_aux, gen2.param_bucket.flat)
        assert all(_same_bits(x, y) for x, y in zip(want[i], got)), i
    if adversarial:
        assert torch.equal(disc.param_bucket.flat, disc2.param_bucket.flat)
    assert not _same_bits(want[0][-3], want[2][-3])                     # the term's values moved with the parameters
    assert GraphedTrainStep(gen2, og2, B, L, disc2, od2, dropout=False).last_aux is None


def test_adversarial_step_takes_aux(clips):
    from cmgan_amd.synth import discriminator_state_dict
    from cmgan_amd.training import AdamW, AuxLoss, DiscriminatorTrain, adversarial_train_step
    clean, noisy = clips
    pesq = torch.tensor([0.4, 0.7], device=DEV)
    aux = AuxLoss((256, 1024), w_mr=0.5, w_si=0.02)

    def run(aux):
        gen, og = _fresh()
        disc = DiscriminatorTrain(discriminator_state_dict(0), engine=gen.engine)
        od = AdamW(gen.engine, disc.param_bucket, disc.grad_bucket, lr=1e-3)
        out = adversarial_train_step(gen, disc, og, od, clean, noisy, pesq, masks=None, disc_masks=None, update=False, aux=aux)
        return out, gen.grad_bucket.flat.clone(), gen.last_aux

    (l0, t0, g0, d0), grads0, none = run(None)
    (l1, t1, g1, d1), grads1, last = run(aux)
    (l2, t2, g2, d2), grads2, _ = run(AuxLoss())
    assert none is None and _same_bits(l2, l0) and _same_bits(grads2, grads0) and _same_bits(d2, d0)
    assert _same_bits(t1, t0) and _same_bits(g1, g0) and _same_bits(l1, l0 + last[0][0]) and not torch.equal(grads1, grads0)
