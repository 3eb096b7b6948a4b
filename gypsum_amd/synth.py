"""Deterministic synthetic GPS L1 C/A baseband IQ (host side, numpy).

There is no recording available offline, so every parity test and
the benchmark run on IQ made here.  The signal model follows SURVEY section 8(d2):

    x[n] = sum_sv  a * prn_sv[(n - cp) mod N] * bit_sv(n) * exp(1j*(2*pi*d*n/fs + phi))
           + sigma * (N(0,1) + 1j*N(0,1))

cast to complex64, i.e. the interleaved-float32 GNU Radio format the reference
reads (antenna_sample_provider.py:112-119).  A satellite placed at code phase
``cp`` produces its correlation peak at index ``cp`` of
``frequency_domain_correlation`` (utils.py:59-73).

Amplitudes must respect the reference tracker's un-normalised loop gains
(SURVEY F6): a*N of roughly 20-40 and sigma about 6*a.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from .gps_ca_prn_codes import generate_ca_code_table


@dataclass
class SyntheticSatellite:
    sat_id: int                # 1..32
    doppler_hz: float
    code_phase: int            # samples, 0..N-1
    carrier_phase: float       # radians
    amplitude: float
    nav_bits: Optional[np.ndarray] = None   # +-1 per 20 ms, None -> all +1
    nav_bit_offset_ms: int = 0              # ms into the first bit at n = 0


@dataclass
class SyntheticScene:
    fs: int
    n_ms: int
    sats: List[SyntheticSatellite]
    noise_sigma: float
    seed: int
    samples_per_ms: int = field(init=False)

    def __post_init__(self) -> None:
        if self.fs % 1_023_000:
            raise ValueError("sample rate must be an integer multiple of 1.023 MHz (SURVEY F1)")
        self.samples_per_ms = self.fs // 1000


def default_amplitudes(fs: int) -> tuple[float, float]:
    """(a, sigma) such that a*N ~ 20-40 and sigma ~ 5-6 a  (SURVEY section 8 d2 / F6)."""
    n = fs // 1000
    a = round(20.46 / n, 6) if n <= 4092 else round(40.92 / n, 6)
    return a, round(a * (5.0 if n <= 4092 else 6.0), 6)


def random_scene(fs: int, n_ms: int, n_sats: int, seed: int, max_doppler: float = 4500.0,
                 max_code_phase: Optional[int] = None, with_nav_bits: bool = True,
                 amplitude: Optional[float] = None, noise_sigma: Optional[float] = None) -> SyntheticScene:
    """Draw `n_sats` visible satellites (without replacement) with uniform Doppler / code phase / carrier phase."""
    rng = np.random.default_rng(seed)
    n = fs // 1000
    a, sg = default_amplitudes(fs)
    a = amplitude if amplitude is not None else a
    sg = noise_sigma if noise_sigma is not None else sg
    ids = rng.choice(np.arange(1, 33), size=n_sats, replace=False)
    sats = []
    for sv in ids:
        n_bits = n_ms // 20 + 2
        sats.append(SyntheticSatellite(
            sat_id=int(sv),
            doppler_hz=float(rng.uniform(-max_doppler, max_doppler)),
            code_phase=int(rng.integers(0, max_code_phase if max_code_phase else n)),
            carrier_phase=float(rng.uniform(0, 2 * np.pi)),
            amplitude=a,
            nav_bits=(rng.integers(0, 2, n_bits) * 2 - 1).astype(np.int8) if with_nav_bits else None,
            nav_bit_offset_ms=int(rng.integers(0, 20)) if with_nav_bits else 0,
        ))
    return SyntheticScene(fs=fs, n_ms=n_ms, sats=sats, noise_sigma=sg, seed=seed + 1)


def lock_regime_scene(fs: int, n_ms: int, seed: int) -> SyntheticScene:
    """A scene in which `is_locked()` (tracker.py:157-203) is REACHABLE.

    The lock test compares absolute variances of the un-normalised prompt peaks: var(last 250 I*Q) < 900 and the mean of the two
    poles' var(I) < 2 (config.py:25-27, tracker.py:170-186).  With peak ~ a*N and per-component noise variance v = sigma^2 * N
    (plus ~(a*N)^2 / 2046 per interfering satellite), that is v < 2 and (a*N)^2 * v < 900: SURVEY section 8 d2's sigma = 6a puts
    v at 5.1 (2.046 Msps) / 7.4 (8.184 Msps), where no channel can ever lock.  Here a*N ~ U(14, 27), v ~ U(0.05, 1.7) and
    2-4 satellites: most channels lock once the 250-ms window has filled (the regime a receiver that reaches a position fix
    lives in), those near (a*N)^2 * v ~ 900 flap between the 3-Hz and 6-Hz loops, some never lock."""
    rng = np.random.default_rng([seed, 0x10C4ED])
    n = fs // 1000
    n_sats = int(rng.integers(2, 5))
    a_n = float(rng.uniform(14.0, 27.0))
    v = float(rng.uniform(0.05, 1.7))
    return random_scene(fs, n_ms, n_sats, seed, max_code_phase=(2046 if n > 2046 else None),
                        amplitude=a_n / n, noise_sigma=float(np.sqrt(v / n)))


def render(scene: SyntheticScene, block_ms: int = 50) -> np.ndarray:
    """complex64[n_ms * N].  float64 synthesis, complex64 storage; deterministic in `scene.seed`."""
    n = scene.samples_per_ms
    fs = scene.fs
    chips = generate_ca_code_table()
    up = n // 1023
    out = np.empty(scene.n_ms * n, dtype=np.complex64)
    rng = np.random.default_rng(scene.seed)
    replicas: Dict[int, np.ndarray] = {}
    for s in scene.sats:
        rep = np.repeat(chips[s.sat_id - 1].astype(np.float64) * 2 - 1, up)
        replicas[s.sat_id] = np.roll(rep, s.code_phase)
    for b0 in range(0, scene.n_ms, block_ms):
        b1 = min(scene.n_ms, b0 + block_ms)
        idx = np.arange(b0 * n, b1 * n, dtype=np.float64)
        acc = np.zeros((b1 - b0) * n, dtype=complex)
        for s in scene.sats:
            code = np.tile(replicas[s.sat_id], b1 - b0)
            sig = s.amplitude * code * np.exp(1j * (2 * np.pi * s.doppler_hz * idx / fs + s.carrier_phase))
            if s.nav_bits is not None:
                ms = np.arange(b0, b1) + s.nav_bit_offset_ms
                bits = s.nav_bits[(ms // 20) % len(s.nav_bits)].astype(np.float64)
                sig = sig * np.repeat(bits, n)
            acc += sig
        noise = rng.standard_normal((b1 - b0) * n) + 1j * rng.standard_normal((b1 - b0) * n)
        acc += scene.noise_sigma * noise
        out[b0 * n:b1 * n] = acc.astype(np.complex64)
    return out


def render_at_rate(scene: SyntheticScene, fs: int, block_ms: int = 50) -> np.ndarray:
    """The continuous-time model of `render` sampled at any rate `fs` (whole kHz; e.g. 4 Msps): complex64[n_ms * fs / 1000].

    Satellite s's code delay is tau = s.code_phase / scene.fs seconds (chip floor((t - tau) * 1.023e6) at t = n / fs), its carrier
    exp(1j * (2 pi d t + phi)) and its data bit that of receiver millisecond floor(t * 1000), exactly as `render` has them at
    t = n / scene.fs; the noise is complex white with sigma `scene.noise_sigma` per component and sample at `fs`.  Resampled to
    scene.fs, satellite s therefore acquires at code phase round(tau * scene.fs) = s.code_phase."""
    fs = int(fs)
    if fs % 1000:
        raise ValueError("fs must be a whole number of kHz")
    n = fs // 1000
    chips = generate_ca_code_table().astype(np.float64) * 2 - 1
    out = np.empty(scene.n_ms * n, dtype=np.complex64)
    rng = np.random.default_rng([scene.seed, fs])
    for b0 in range(0, scene.n_ms, block_ms):
        b1 = min(scene.n_ms, b0 + block_ms)
        acc = _signal_at_rate(scene, fs, chips, b0, b1)
        acc += scene.noise_sigma * (rng.standard_normal((b1 - b0) * n) + 1j * rng.standard_normal((b1 - b0) * n))
        out[b0 * n:b1 * n] = acc.astype(np.complex64)
    return out


def _signal_at_rate(scene: SyntheticScene, fs: int, chips: np.ndarray, b0: int, b1: int) -> np.ndarray:
    """render_at_rate's noiseless model, complex128, for receiver milliseconds b0 .. b1-1 at rate fs."""
    n = fs // 1000
    idx = np.arange(b0 * n, b1 * n, dtype=np.int64)
    t = idx / fs
    ms = idx // n                                          # receiver millisecond of each sample (exact)
    acc = np.zeros((b1 - b0) * n, dtype=complex)
    for s in scene.sats:
        # chip index floor((t - tau) * 1.023e6) in exact integer arithmetic: (idx * scene.fs - cp * fs) * 1023 // (fs * scene.fs / 1000)
        num = (idx * scene.fs - s.code_phase * fs) * 1023
        chip = np.floor_divide(num, fs * (scene.fs // 1000)) % 1023
        sig = s.amplitude * chips[s.sat_id - 1][chip] * np.exp(1j * (2 * np.pi * s.doppler_hz * t + s.carrier_phase))
        if s.nav_bits is not None:
            sig = sig * s.nav_bits[((ms + s.nav_bit_offset_ms) // 20) % len(s.nav_bits)].astype(np.float64)
        acc += sig
    return acc


def render_real_if(scene: SyntheticScene, fs: int, if_hz: int, block_ms: int = 50) -> np.ndarray:
    """The real recording of a front end with its band at `if_hz` (signed, whole Hz), sampled at `fs`: float64[n_ms * fs / 1000].

    The signal is 2 Re{s(t) exp(j 2 pi if_hz t)}, s being render_at_rate's noiseless model at fs (the IF carrier's phase reduced
    exactly, ((if_hz * n) mod fs) / fs turns at sample n), so a negative if_hz gives the inverted spectrum with no special case.  The
    noise is real white Gaussian with sigma sqrt(2) * scene.noise_sigma: down-converted (gain 1/2 on the signal and on the noise's
    power spectral density), the stream has the C/N0 of render_at_rate(scene, fs)."""
    fs, if_hz = int(fs), int(if_hz)
    if fs % 1000:
        raise ValueError("fs must be a whole number of kHz")
    n = fs // 1000
    chips = generate_ca_code_table().astype(np.float64) * 2 - 1
    out = np.empty(scene.n_ms * n, dtype=np.float64)
    rng = np.random.default_rng([scene.seed, fs, 1])
    f = if_hz % fs
    for b0 in range(0, scene.n_ms, block_ms):
        b1 = min(scene.n_ms, b0 + block_ms)
        idx = np.arange(b0 * n, b1 * n, dtype=np.int64)
        turns = ((idx % fs) * f % fs).astype(np.float64) / fs
        acc = 2.0 * (_signal_at_rate(scene, fs, chips, b0, b1) * np.exp(2j * np.pi * turns)).real
        acc += np.sqrt(2.0) * scene.noise_sigma * rng.standard_normal((b1 - b0) * n)
        out[b0 * n:b1 * n] = acc
    return out


def nav_symbol_at(sat: SyntheticSatellite, ms: int) -> int:
    """The +-1 data symbol satellite `sat` carries during millisecond `ms` of the scene."""
    if sat.nav_bits is None:
        return 1
    return int(sat.nav_bits[((ms + sat.nav_bit_offset_ms) // 20) % len(sat.nav_bits)])


def kat_grid_scene() -> tuple[np.ndarray, int, int]:
    """The frozen config-2 known-answer input of SURVEY section 8(c5): (iq complex64[2046], fs, N)."""
    fs, n = 2_046_000, 2046
    rng = np.random.default_rng(20260925)
    chips = generate_ca_code_table()
    idx = np.arange(n)
    x = np.zeros(n, dtype=complex)
    for sv, d, cp, phi in ((3, -2500, 100, 0.1), (11, 1500, 1500, 2.0), (22, 4000, 2045, -1.0), (30, 0, 0, 0.5)):
        rep = np.repeat(chips[sv - 1].astype(np.float64) * 2 - 1, 2)
        x += 0.02 * np.roll(rep, cp) * np.exp(1j * (2 * np.pi * d * idx / fs + phi))
    x += 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), fs, n


def write_packed(x: np.ndarray, packing, path, twin_path=None, scale: float | None = None, tail_words: int = 0) -> dict:
    """Write `x` (complex for an I,Q packing, real for a real one) as a packed recording (gypsum_amd.packing), quantized to the
    nearest level of x / scale (scale None: the rms of one component, so the words span the levels), plus `tail_words` words of a
    partial sample at the end (fewer than a sample's words: they are ignored by readers).  With `twin_path`, also write the int8
    recording of the same file's whole samples: each word its level, so the int8 path on the twin gives the packed path's bits.
    Returns {"scale", "file_samples", "bytes"}."""
    from . import packing as pk

    x = np.asarray(x)
    if scale is None:
        comp = np.concatenate([x.real.ravel(), x.imag.ravel()]) if np.iscomplexobj(x) else x.ravel()
        scale = float(np.sqrt(np.mean(comp.astype(np.float64) ** 2))) or 1.0
    codes = pk.quantize(x, packing, scale)
    if tail_words:
        if tail_words >= packing.words_per_sample:
            raise ValueError("tail_words must be fewer than a sample's words")
        codes = np.concatenate([codes, np.full(tail_words, (1 << packing.bits) - 1, dtype=np.int64)])
    data = pk.pack(codes, packing)
    with open(path, "wb") as f:
        f.write(data)
    n = packing.file_samples(len(data))
    if twin_path is not None:
        whole = np.zeros(n * packing.words_per_sample, dtype=np.int64)   # the pad bits of the last byte are code 0 words
        k = min(whole.size, codes.size)
        whole[:k] = codes[:k]
        lv = np.asarray(packing.levels)
        if not np.array_equal(lv, np.rint(lv)) or np.abs(lv).max() > 127:
            raise ValueError("the int8 twin needs integer levels of magnitude <= 127")
        lv.astype(np.int8)[whole].tofile(twin_path)
    return {"scale": scale, "file_samples": n, "bytes": len(data)}


def write_packed_scene(scene: SyntheticScene, fs: int, packing, path, twin_path=None, if_hz: int | None = None,
                       scale: float | None = None) -> dict:
    """A scene as a packed recording at `fs` (render_at_rate for an I,Q packing; render_real_if at `if_hz` for a real one), plus
    its int8 twin (write_packed)."""
    if packing.real:
        if if_hz is None:
            raise ValueError("a real packing needs if_hz")
        x = render_real_if(scene, fs, if_hz)
    else:
        x = render_at_rate(scene, fs)
    return write_packed(x, packing, path, twin_path, scale)
