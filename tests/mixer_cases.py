"""The DynamicMixer cases whose draws, messages and output bits are recorded at one commit and replayed at every later one
(tests/golden/make_mixer_draws.py, make_mixer_bits.py; tests/test_mix_host.py, tests/test_gpu_mix.py), and the helpers both
sides share: one definition of every case, so a recorder and its test cannot drift apart."""
import itertools

import numpy as np
import torch

from cmgan_amd.mixing import ChannelSampler, DynamicMixer, NoiseBank, RirBank, RoomSampler

SEEDS = dict(mixer=11, rooms=12, channel=13)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def assert_recorded_bits(case, got, want):
    """got: device tensors by name; want: the recorded unsigned views.  Names the first differing row and index."""
    for key, t in got.items():
        w = want[f"{case}/{key}"]
        g = t.contiguous().cpu().numpy().view(w.dtype)
        assert g.shape == w.shape, f"{case} {key}: shape {g.shape}, recorded {w.shape}"
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            row, idx = int(at[0]), (int(at[1]) if len(at) > 1 else 0)
            f = np.float32 if w.dtype == np.uint32 else np.float64
            raise AssertionError(f"{case} {key}: row {row} differs first at index {idx}: got {g[tuple(at)]:#x} "
                                 f"({g.view(f)[tuple(at)]!r}), recorded {w[tuple(at)]:#x} ({w.view(f)[tuple(at)]!r})")


def flatten(prefix, value):
    """(name, tensor or None) for a tensor, None, or a (named) tuple of such, names joined with '.'."""
    if value is None or isinstance(value, torch.Tensor):
        return [(prefix, value)]
    names = getattr(value, "_fields", None) or range(len(value))
    return [kv for n, v in zip(names, value) for kv in flatten(f"{prefix}.{n}", v)]


def unsigned(t: torch.Tensor) -> np.ndarray:
    """The tensor's elements as they lie in memory order of a contiguous copy, viewed as unsigned integers of their size."""
    a = t.detach().contiguous().cpu().numpy()
    return a.view(UINT[a.dtype.itemsize])


def generators(device):
    return {k: torch.Generator(device=device).manual_seed(s) for k, s in SEEDS.items()}


# ------------------------------------------------------------------ the draws (CPU): 384 option combinations
DRAW_B = 6
DRAW_AXES = (("rir", ("none", "bank", "rooms")), ("p_reverb", (1.0, 0.5)), ("level_db", (None, (-30.0, -20.0))),
             ("channel", (False, True)), ("speed", (False, True)), ("sources", (None, (0, 2))),
             ("stretch", ("off", "tempo", "pitch", "both")))


def draw_cases():
    """(name, options) of every combination, in a fixed order."""
    for combo in itertools.product(*(values for _, values in DRAW_AXES)):
        opt = dict(zip((k for k, _ in DRAW_AXES), combo))
        yield "/".join(f"{k}={v}" for k, v in opt.items()), opt


def draw_mixer(opt, engine):
    """The mixer of one combination over a three-item noise bank of lengths 100, 50 and 7, and its three generators."""
    dev = engine.device
    gens = generators(dev)
    bank = NoiseBank.from_arrays([np.ones(100, np.float32), np.ones(50, np.float32), np.ones(7, np.float32)], device=dev)
    kw = dict(generator=gens["mixer"], p_reverb=opt["p_reverb"], level_db=opt["level_db"], sources=opt["sources"])
    if opt["rir"] == "bank":
        kw["rir_bank"] = RirBank.from_arrays([[1.0, 0.5], [0.1, 0.9, 0.3, 0.2]], device=dev)
    if opt["rir"] == "rooms":
        kw.update(rooms=RoomSampler(generator=gens["rooms"]), rir_seconds=0.05)
    if opt["channel"]:
        kw["channel"] = ChannelSampler(generator=gens["channel"])
    if opt["speed"]:
        kw.update(speed=(0.9, 1.1), p_speed=0.5)
    if opt["stretch"] in ("tempo", "both"):
        kw.update(tempo=(0.9, 1.1), p_tempo=0.5)
    if opt["stretch"] in ("pitch", "both"):
        kw["pitch"] = (-2.0, 2.0)
    return DynamicMixer(engine, bank, **kw), gens


def drawn_fields(mixer, gens, B=DRAW_B):
    """Everything one case pins: the fields of draw(B) and draw_stretch(B, d.speed), then the generators' final states."""
    d = mixer.draw(B)
    s = mixer.draw_stretch(B, d.speed)
    out = [("type", torch.tensor([ord(c) for c in type(d).__name__], dtype=torch.uint8))] + flatten("draw", d)
    return out + flatten("stretch", s) + [(f"state.{k}", g.get_state()) for k, g in gens.items()]


def pack(fields):
    """[(name, tensor or None)] as (manifest rows, bytes): a row is [name, dtype, shape, strides, byte count], or
    [name, None] for None; the bytes are the tensors' unsigned views, one after the other."""
    rows, parts = [], []
    for name, t in fields:
        if t is None:
            rows.append([name, None])
            continue
        raw = unsigned(t).reshape(-1).view(np.uint8)
        rows.append([name, str(t.dtype), list(t.shape), list(t.stride()), int(raw.size)])
        parts.append(raw)
    return rows, np.concatenate(parts)


# ------------------------------------------------------------------ the messages (CPU): one bad option per parser path
class NoEngine:
    device = torch.device("cpu")


def _mixer(**kw):
    return DynamicMixer(NoEngine(), NoiseBank.from_arrays([np.ones(9, np.float32)]), **kw)


BAD_OPTIONS = [
    ("snr_db reversed", _mixer, dict(snr_db=(5, 1))),
    ("snr_db no pair", _mixer, dict(snr_db=3)),
    ("source_snr_db no pair", _mixer, dict(sources=(0, 2), source_snr_db=3)),
    ("source_snr_db reversed", _mixer, dict(sources=(0, 2), source_snr_db=[5, 1])),
    ("sources no pair", _mixer, dict(sources=3)),
    ("sources three", _mixer, dict(sources=(0, 1, 2))),
    ("sources fraction", _mixer, dict(sources=(0, 1.5))),
    ("sources bool", _mixer, dict(sources=(False, 2))),
    ("sources five", _mixer, dict(sources=[0, 5])),
    ("sources none used", _mixer, dict(sources=(0, 0))),
    ("speed no pair", _mixer, dict(speed=1.1)),
    ("speed out of range", _mixer, dict(speed=[1, 5])),
    ("level_db no pair", _mixer, dict(level_db="loud")),
    ("level_db reversed", _mixer, dict(level_db=[-20, -30])),
    ("level_db infinite", _mixer, dict(level_db=(-float("inf"), -30))),
    ("tempo no pair", _mixer, dict(tempo=(0.9,))),
    ("tempo out of range", _mixer, dict(tempo=[0.2, 1])),
    ("pitch no pair", _mixer, dict(pitch=2)),
    ("pitch out of range", _mixer, dict(pitch=[-13, 0])),
    ("p_reverb", _mixer, dict(p_reverb=1.5)),
    ("p_speed", _mixer, dict(p_speed=-0.1)),
    ("p_tempo", _mixer, dict(p_tempo=float("nan"))),
    ("p_pitch", _mixer, dict(p_pitch=2)),
    ("stretch_hop", _mixer, dict(stretch_hop=15)),
    ("stretch_hop fraction", _mixer, dict(stretch_hop=64.5)),
    ("stretch_search", _mixer, dict(stretch_search=1025)),
    ("stretch_search bool", _mixer, dict(stretch_search=True)),
    ("stretch rates", _mixer, dict(tempo=(3.0, 3.5), pitch=(-6, 0))),
    ("warp rates", _mixer, dict(speed=(3.0, 3.5), pitch=(0, 6))),
    ("early_ms", _mixer, dict(early_ms=-1)),
    ("rir_seconds", _mixer, dict(rooms=RoomSampler(), rir_seconds=5.0)),
    ("rir_seconds images", _mixer, dict(rooms=RoomSampler(dims=((0.05, 3.0, 2.5), (10.0, 8.0, 4.0)), margin=0.0), rir_seconds=0.5)),
    ("rooms and rir_bank", _mixer, dict(rooms=RoomSampler(), rir_bank=RirBank.from_arrays([[1.0]]))),
    ("snr_on", _mixer, dict(snr_on="peak")),
    ("sample_rate for levels", _mixer, dict(snr_on="active", sample_rate=4000)),
    ("channel_on", _mixer, dict(channel_on="target")),
    ("channel type", _mixer, dict(channel=dict())),
    ("source_bank without sources", _mixer, dict(source_bank=NoiseBank.from_arrays([np.ones(3, np.float32)]))),
    ("dry_noise without sources", _mixer, dict(dry_noise=False)),
    # several wrong at once: the first in the constructor's order is the one reported
    ("order: sources before speed", _mixer, dict(sources=3, speed=1.1)),
    ("order: speed before tempo", _mixer, dict(speed=1.1, tempo=1.1)),
    ("order: p_speed before tempo", _mixer, dict(p_speed=2, tempo=1.1)),
    ("order: tempo before pitch", _mixer, dict(tempo=1.1, pitch=2)),
    ("order: pitch before p_tempo", _mixer, dict(pitch=2, p_tempo=2)),
    ("order: p_pitch before stretch_hop", _mixer, dict(p_pitch=2, stretch_hop=1)),
    ("order: stretch_search before channel_on", _mixer, dict(stretch_search=-1, channel_on="x")),
    ("order: channel before snr_on", _mixer, dict(channel=3, snr_on="x")),
    ("order: snr_on before level_db", _mixer, dict(snr_on="x", level_db=3)),
    ("order: level_db before snr_db", _mixer, dict(level_db=3, snr_db=(5, 1))),
    ("order: snr_db before p_reverb", _mixer, dict(snr_db=(5, 1), p_reverb=2)),
    ("order: p_reverb before early_ms", _mixer, dict(p_reverb=2, early_ms=-1)),
    ("channel p_highpass", ChannelSampler, dict(p_highpass=1.5)),
    ("channel p_bandlimit", ChannelSampler, dict(p_bandlimit=-1)),
    ("channel p_clip", ChannelSampler, dict(p_clip=float("nan"))),
    ("channel highpass_hz no pair", ChannelSampler, dict(highpass_hz=20.0)),
    ("channel highpass_hz zero", ChannelSampler, dict(highpass_hz=[0, 120])),
    ("channel eq_hz reversed", ChannelSampler, dict(eq_hz=(500.0, 50.0))),
    ("channel eq_q infinite", ChannelSampler, dict(eq_q=(0.5, float("inf")))),
    ("channel bandlimit_hz no pair", ChannelSampler, dict(bandlimit_hz=("a", "b"))),
    ("channel clip_rel", ChannelSampler, dict(clip_rel=(0.0, 0.9))),
    ("channel order: probability before range", ChannelSampler, dict(p_clip=2, highpass_hz=1)),
    ("rooms rt60 no pair", RoomSampler, dict(rt60=0.5)),
    ("rooms rt60 reversed", RoomSampler, dict(rt60=[0.8, 0.2])),
    ("rooms dims", RoomSampler, dict(dims=(3.0, 10.0))),
    ("rooms margin", RoomSampler, dict(margin=2.0)),
]


def message_of(make, kw):
    """[exception type's name, its full text] of make(**kw), which has to raise."""
    try:
        make(**kw)
    except Exception as e:
        return [type(e).__name__, str(e)]
    raise AssertionError(f"{make.__name__}({kw}) raised nothing")


# ------------------------------------------------------------------ the outputs (GPU): 12 configurations
BITS_B, BITS_L = 3, 1536


def _decaying(rng, n):
    return (rng.standard_normal(n) * np.exp(-np.arange(n) / (0.2 * n + 1.0))).astype(np.float32)


def bits_inputs(engine):
    """The clean batch and the banks of every configuration, from fixed numpy seeds (nothing of them is stored)."""
    rng = np.random.default_rng(1812)
    dev = engine.device
    clean = torch.from_numpy((0.1 * rng.standard_normal((BITS_B, BITS_L))).astype(np.float32)).to(dev)
    noise = NoiseBank.from_arrays([(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (4000, 900, 7)], device=dev)
    talkers = NoiseBank.from_arrays([(0.2 * rng.standard_normal(n)).astype(np.float32) for n in (2500, 1000)], device=dev)
    rirs = RirBank.from_arrays([_decaying(rng, 300), _decaying(rng, 120)], device=dev)
    return clean, noise, talkers, rirs


def bits_configs(engine):
    """(name, mixer) of the 12 configurations, each with generators of its own at the fixed seeds."""
    clean, noise, talkers, rirs = bits_inputs(engine)
    speed = dict(speed=(0.9, 1.1), p_speed=0.5)
    stretch = dict(stretch_hop=64, stretch_search=40)
    options = [
        ("defaults", lambda g: dict()),
        ("rir_bank", lambda g: dict(rir_bank=rirs, p_reverb=0.5, early_ms=20)),
        ("rooms", lambda g: dict(rooms=RoomSampler(generator=g["rooms"]), rir_seconds=0.02)),
        ("active+level", lambda g: dict(snr_on="active", level_db=(-30, -20))),
        ("channel", lambda g: dict(channel=ChannelSampler(generator=g["channel"]), channel_on="both")),
        ("speed", lambda g: dict(**speed)),
        ("tempo", lambda g: dict(tempo=(0.9, 1.1), **stretch)),
        ("pitch", lambda g: dict(pitch=(-2, 2), **stretch)),
        ("tempo+pitch+speed", lambda g: dict(tempo=(0.9, 1.1), p_tempo=0.5, pitch=(-2, 2), **speed, **stretch)),
        ("sources+rir_bank", lambda g: dict(sources=(0, 2), rir_bank=rirs)),
        ("sources+rooms", lambda g: dict(sources=(1, 2), rooms=RoomSampler(generator=g["rooms"]), rir_seconds=0.02,
                                         dry_noise=False, snr_on="active")),
        ("everything", lambda g: dict(rooms=RoomSampler(generator=g["rooms"]), rir_seconds=0.02, p_reverb=0.5, early_ms=20,
                                      snr_on="active", level_db=(-30, -20), channel=ChannelSampler(generator=g["channel"]),
                                      channel_on="both", tempo=(0.9, 1.1), p_tempo=0.5, pitch=(-2, 2), **speed, **stretch,
                                      sources=(0, 2), source_bank=talkers, source_snr_db=(0, 10))),
    ]
    for name, kw in options:
        g = generators(engine.device)
        yield name, DynamicMixer(engine, noise, generator=g["mixer"], **kw(g)), clean


def mixed_fields(mixer, clean):
    """Everything one configuration pins: target, noisy, the info vectors, last_draw, last_stretch and last_level."""
    target, noisy, info = mixer(clean)
    out = [("target", target), ("noisy", noisy)] + flatten("info", info) + flatten("draw", mixer.last_draw)
    out += flatten("stretch", mixer.last_stretch) + flatten("level", mixer.last_level)
    return out
