#!/usr/bin/env python3
"""Measure the default z threshold of GpsSatelliteDetector.detect_weak_satellites_in_antenna_data.

The threshold cannot be derived in closed form: the largest z of a noise-only search is the maximum of 32 x bins x N correlated
chi-square sums.  This script runs the float64 CPU model (tests/hybrid_model.py: no GPU) on noise-only input at the default
configuration -- 2.046 Msps, coherent_ms = 10, GYP_HYB_ALTERNATE | GYP_HYB_CODE_DOPPLER, 200 ms (20 blocks), +-7 kHz coarse and the
10 Hz fine level, all 32 satellites -- over `--seeds` seeds (default 8) and prints the largest z of each and the default
threshold, that maximum x 1.25 (a quarter of margin because eight seeds sample the tail thinly).  About 20 s per seed and core.

    python tools/hybrid_threshold.py [--seeds 8] [--first-seed 1] [--jobs 4]
"""
from __future__ import annotations

import argparse
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

FS, N, T, N_MS = 2_046_000, 2046, 10, 200
MARGIN = 1.25


def largest_noise_z(seed: int) -> float:
    import hybrid_model as hm

    rng = np.random.default_rng([seed, 0x7E57])
    x = (rng.standard_normal(N_MS * N) + 1j * rng.standard_normal(N_MS * N)).astype(np.complex64)   # z does not depend on the noise level
    res = hm.acquire_weak(x, FS, N, range(1, 33), T, N_MS // T, hm.ALTERNATE | hm.CODE_DOPPLER, 0.0, 7000.0, 10.0)
    return max(r.z for r in res)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--first-seed", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    if a.seeds < 8:
        ap.error("at least 8 seeds")
    seeds = list(range(a.first_seed, a.first_seed + a.seeds))
    with ProcessPoolExecutor(max_workers=max(1, a.jobs)) as pool:
        zs = list(pool.map(largest_noise_z, seeds))
    for s, z in zip(seeds, zs):
        print(f"seed {s}: largest z {z:.4f}")
    print(f"largest of {len(seeds)} seeds: {max(zs):.4f}; x {MARGIN} = {max(zs) * MARGIN:.4f}")


if __name__ == "__main__":
    main()
