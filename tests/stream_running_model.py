"""CPU restatement of the RUNNING-statistics streaming contract (include/cmgan_hip.h, "Streaming";
cmgan_amd/streaming.py, stats_mode="running").  TEST INFRASTRUCTURE ONLY; float32 like oracle/cmgan_oracle.py.

The frozen contract (oracle/stream_oracle.py) normalises every generator InstanceNorm with a statistics set calibrated up
front.  The running contract carries, per norm and per (row, channel), fp64 sums n, sum(x), sum(x^2) of that norm's
INPUT.  Each call of a norm adds its input over the step's NEW frames (history frames in front are not counted again),
sets mean = S1 / n and var = max(S2 / n - mean^2, 0) (in_finalize_kernel's arithmetic) and normalises ALL frames of the
call with that pair.  The step rule itself - which frames the encoder, the TSCBs and the decoders see - is
stream_oracle.stream_forward's, reused as is: `running_stats` swaps in the norm and tells it where a call's new frames
start.
"""
import torch

from oracle import cmgan_oracle as O
from oracle import stream_oracle as S


class running_stats:
    """Context manager: every generator InstanceNorm (cmgan_oracle._instance_norm, its single call site) uses the
    running rule of the module header.  `sums` {norm prefix: (n, S1 [B,C] fp64, S2 [B,C] fp64)} is updated in place;
    `new_from` is the index of the first new frame of the next norm calls.  Inside, stream_oracle's encoder / decoder
    stages are wrapped so the index follows stream_forward's step rule: the encoder's k-th call covers
    [max(e0 - 15, 0), e1) with e0 the frames encoded so far, the decoders' [max(lo - 15, 0), lo + n) with lo the frames
    decoded so far."""

    def __init__(self, sums: dict | None = None):
        self.sums = {} if sums is None else sums
        self.new_from = 0
        self.enc_seen = 0
        self.dec_seen = 0

    def norm(self, x, w, b, key):
        xd = x[:, :, self.new_from:].double()
        n0, s1, s2 = self.sums.get(key, (0, 0.0, 0.0))
        n = n0 + xd.shape[2] * xd.shape[3]
        s1 = s1 + xd.sum(dim=(2, 3))
        s2 = s2 + (xd * xd).sum(dim=(2, 3))
        self.sums[key] = (n, s1, s2)
        mean = s1 / n
        var = torch.clamp(s2 / n - mean * mean, min=0.0)
        mean = mean.float()[:, :, None, None]
        var = var.float()[:, :, None, None]
        return (x - mean) / torch.sqrt(var + O.EPS) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)

    def _encoder(self, sd, spec):
        h0 = max(self.enc_seen - S.HIST, 0)
        self.new_from = self.enc_seen - h0
        self.enc_seen = h0 + spec.size(2)
        return self._enc(sd, spec)

    def _decoders(self, sd, h, spec):
        d0 = max(self.dec_seen - S.HIST, 0)
        self.new_from = self.dec_seen - d0
        self.dec_seen = d0 + spec.size(2)
        return self._dec(sd, h, spec)

    def __enter__(self):
        self._norm, self._enc, self._dec = O._instance_norm, S._encoder, S._decoders
        O._instance_norm, S._encoder, S._decoders = self.norm, self._encoder, self._decoders
        return self

    def __exit__(self, *exc):
        O._instance_norm, S._encoder, S._decoders = self._norm, self._enc, self._dec


@torch.no_grad()
def stream_forward(sd, spec, window: int, context: int, lookahead: int, sums: dict | None = None):
    """spec [B,2,T,F] -> (est_real, est_imag) [B,1,T,F]: stream_oracle.stream_forward's steps, running statistics."""
    with running_stats(sums):
        return S.stream_forward(sd, spec, {}, window, context, lookahead)


@torch.no_grad()
def encoder_step(sd, spec, hist: int, sums: dict):
    """One encoder step on spec [B,2,t,F] whose first `hist` frames were counted before: the dense encoder's output."""
    with running_stats(sums) as r:
        r.new_from = hist
        return r._enc(sd, spec)


@torch.no_grad()
def enhance_stream(sd, noisy, window: int = 400, context: int = 40, lookahead: int = 40, n_fft: int = 400,
                   hop: int = 100):
    """noisy [B, L] -> enhanced [B, hop (T - 1)]: stream_oracle.enhance_stream without the calibration pass."""
    c = O.rms_scale(noisy)
    spec = O.stft_compress(noisy * c[:, None], n_fft, hop)
    real, imag = stream_forward(sd, spec, window, context, lookahead)
    return O.uncompress_istft(real, imag, n_fft, hop) / c[:, None]
