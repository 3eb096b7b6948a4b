"""The end-to-end scene of the weak-signal acquisition tests (tests/test_hybrid_host.py gates it on the float64 model alone,
tests/test_gpu_hybrid.py runs the device on it) and the model's answers on it, computed once per process.

2.046 Msps, 220 ms, code Doppler rendered (hybrid_model.render).  Noise sigma 0.05 per component, amplitudes from it through
quality.cn0_of_scene's relation a = sigma sqrt(2 10^(cn0 / 10) / (1000 N)):

    satellite  C/N0      Doppler    code phase  bit offset
    7          30 dB-Hz  +4487 Hz   0           5 ms   (bit edges at 15, 35, ... ms: inside the ODD 10-ms blocks only)
    19         30 dB-Hz  -4462 Hz   N - 1       10 ms  (a multiple of 10: edges on block boundaries)
    26         30 dB-Hz  +1233 Hz   700         13 ms
    3          45 dB-Hz  -2871 Hz   1391        8 ms

SEED = 322 was chosen (`python tests/hybrid_scene.py <seed> ...` prints every gated figure for a seed) so that the gates of
tests/test_hybrid_host.py all hold on the model: among them that satellite 7's random data bits flip at 7 or more of its 11 edges
(at all 11 with this seed) -- with fewer flips summing all 22 blocks beats summing the 11 clean ones, and GYP_HYB_ALTERNATE would
not matter on this scene -- and that the best bin of every present satellite leads its runner-up by more than 1e-3 in z, so that
float32 cannot reorder them on the device.  The model's figures at this seed: z 33.06 / 39.14 / 30.30 / 569.9 (satellites 7, 19,
26, 3), at most 10.24 for the 28 absent satellites; without CODE_DOPPLER 23.77 / 30.96 for 7 and 19, without ALTERNATE 21.71 for 7;
the reference search on the first 10 ms gives the weak ones strengths 1.80, 1.78, 1.85.  tests/golden/hybrid_scene.npz records the
model's 32 answers (`--write-golden`).
"""
from __future__ import annotations

import functools
import math
from pathlib import Path
from typing import Dict, List

import numpy as np

import hybrid_model as hm
from gypsum_amd import synth
from gypsum_amd.quality import cn0_of_scene
from oracle import gypsum_oracle as orc

FS, N, N_MS = 2_046_000, 2046, 220
T, M = 10, 22
FLAGS = hm.ALTERNATE | hm.CODE_DOPPLER
SIGMA = 0.05
SPREAD_HZ, FINE_STEP_HZ = 7000.0, 10.0
SEED = 322
WEAK = (7, 19, 26)
STRONG = (3,)
ALL_SATS = tuple(range(1, 33))


def amplitude(cn0_dbhz: float) -> float:
    a = SIGMA * math.sqrt(2.0 * 10.0 ** (cn0_dbhz / 10.0) / (1000.0 * N))
    assert abs(cn0_of_scene(a, SIGMA, N) - cn0_dbhz) < 1e-9
    return a


def scene(seed: int = SEED) -> synth.SyntheticScene:
    rng = np.random.default_rng([seed, 0x4B1D])
    n_bits = N_MS // 20 + 2
    spec = ((7, 30.0, 4487.0, 0, 5), (19, 30.0, -4462.0, N - 1, 10), (26, 30.0, 1233.0, 700, 13), (3, 45.0, -2871.0, 1391, 8))
    sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=d, code_phase=cp, carrier_phase=float(rng.uniform(0, 2 * np.pi)),
                                     amplitude=amplitude(cn0), nav_bits=(rng.integers(0, 2, n_bits) * 2 - 1).astype(np.int8),
                                     nav_bit_offset_ms=off) for sv, cn0, d, cp, off in spec]
    return synth.SyntheticScene(fs=FS, n_ms=N_MS, sats=sats, noise_sigma=SIGMA, seed=seed)


def truth(seed: int = SEED) -> Dict[int, synth.SyntheticSatellite]:
    return {s.sat_id: s for s in scene(seed).sats}


@functools.lru_cache(maxsize=2)
def iq(seed: int = SEED) -> np.ndarray:
    x = hm.render(scene(seed), code_doppler=True)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)
def model_results(seed: int = SEED) -> Dict[int, hm.WeakResult]:
    """The model's two-level search over all 32 satellites (T = 10, M = 22, both flags), by satellite id."""
    res = hm.acquire_weak(iq(seed), FS, N, ALL_SATS, T, M, FLAGS, 0.0, SPREAD_HZ, FINE_STEP_HZ)
    return {r.sat_id: r for r in res}


def flips_at_edges(sat: synth.SyntheticSatellite) -> int:
    """Data-bit transitions of `sat` inside the scene."""
    sym = [synth.nav_symbol_at(sat, ms) for ms in range(N_MS)]
    return sum(1 for a, b in zip(sym, sym[1:]) if a != b)


def z_at_truth(seed: int, sat: int, flags: int, m: int = M) -> float:
    """The model's z of the cell at the satellite's final model bin (so the flags are compared on one and the same bin)."""
    f = model_results(seed)[sat].doppler_hz
    return hm.hybrid_cell(iq(seed), FS, N, sat, f, T, m, flags).z


def report(seed: int) -> None:
    tr = truth(seed)
    res = model_results(seed)
    rest = [res[s].z for s in ALL_SATS if s not in tr]
    print(f"seed {seed}: largest z of the 28 absent satellites {max(rest):.3f}")
    for sv, s in tr.items():
        r = res[sv]
        print(f"  sat {sv}: z {r.z:.2f} doppler {r.doppler_hz:.1f} (true {s.doppler_hz}) code phase {r.code_phase} (true {s.code_phase}) set {r.set} "
              f"flips {flips_at_edges(s)} margin {r.z_margin:.3g}")
        print(f"     z both flags {z_at_truth(seed, sv, FLAGS):.3f}  no CODE_DOPPLER {z_at_truth(seed, sv, hm.ALTERNATE):.3f}  "
              f"no ALTERNATE {z_at_truth(seed, sv, hm.CODE_DOPPLER):.3f}")
    x10 = iq(seed)[:10 * N]
    replicas = {sv: orc.prn_as_complex(orc.generate_ca_codes()[sv - 1], N) for sv in tr}
    for sv in tr:
        r = orc.acquire_satellite(sv, x10, FS, N, replicas[sv])
        print(f"  reference search, first 10 ms, sat {sv}: strength {r.correlation_strength:.3f} code phase {r.prn_phase_shift} doppler {r.doppler_shift}")


GOLDEN = Path(__file__).resolve().parent / "golden" / "hybrid_scene.npz"
GOLDEN_FIELDS = ("sat_id", "doppler_hz", "code_phase", "carrier_phase", "z", "peak_ratio", "set", "coarse_doppler_hz", "z_margin")


def golden_arrays(res: Dict[int, hm.WeakResult]) -> Dict[str, np.ndarray]:
    return {k: np.array([getattr(res[sv], k) for sv in ALL_SATS]) for k in GOLDEN_FIELDS}


def golden_results() -> Dict[int, hm.WeakResult]:
    """model_results() of SEED as recorded in tests/golden/hybrid_scene.npz (`python tests/hybrid_scene.py --write-golden`;
    tests/test_hybrid_host.py holds the file to the model run afresh), for the GPU tests: the 20-second model search is not theirs
    to repeat."""
    with np.load(GOLDEN) as g:
        assert int(g["seed"]) == SEED
        cols = {k: g[k] for k in GOLDEN_FIELDS}
    return {int(cols["sat_id"][i]): hm.WeakResult(*(cols[k][i].item() for k in GOLDEN_FIELDS)) for i in range(len(ALL_SATS))}


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--write-golden"]:
        np.savez(GOLDEN, seed=SEED, **golden_arrays(model_results()))
        print(f"wrote {GOLDEN}")
    else:
        for a in sys.argv[1:] or [str(SEED)]:
            report(int(a))
