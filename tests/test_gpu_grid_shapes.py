"""The flat grids at the shapes bench.py LAUNCHES them, against the float64 oracle.

tests/test_gpu_parity.py checks the grid kernels on 3 x 3 and 11 x 3 cells; the figures in the bench line come from launches of
8192 units x 640 cells (cfg2), 4096 units x 640 cells + the device's best-bin selection (cfg4) and 4 streams x 32 x 200 cells x 10 ms
coherent (cfg5: 38 400 branch-run work items + grid_merge_parts_kernel).  Here the same launches -- the same device-generated
inputs (gyp_synth_iq_dev, as bench.run_grid / bench.run_cfg5 make them), the same entry points, the same sizes -- are compared with
the reference arithmetic: acquisition.py:154-190 (`get_best_doppler_shift_estimation`) for the non-coherent grids, utils.py:77-108
(`integrate_correlation_with_doppler_shifted_prn`, Coherent) for config 5.  The oracle runs in a pool of worker processes on the
samples downloaded from the device.

Bar: arg-max (code phase) and best bin bit-exact, peak magnitude and strength within 1e-4.  Where the REFERENCE's own two largest
float64 values (two lags of a profile, or two bins' maxima) are closer than GAP = 2e-6 relative, float32 magnitudes (3e-7) may
order them the other way: such a cell is accepted only on the oracle's own margin, counted and printed (the flat grids have no
float64 tie-break; the 10-level search has one).
"""
from __future__ import annotations

import multiprocessing as mp
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import pytest

import survey_worker
from gypsum_amd._lib import BEST_BIN, CELL, GYP_COHERENT, GYP_NON_COHERENT

REPO = Path(__file__).resolve().parents[1]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

GAP = 2e-6
ALL_IDS = list(range(1, 33))


def _shm_dir() -> str:
    return "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()


def _noncoherent_grid(eng, B, T, seed, rng_seed, refined=False):
    """bench.run_grid's launch: B streams x T ms at 2.046 Msps, every (stream, ms) a unit of stride N, 32 satellites x range(-5000, 5000, 500)."""
    import bench

    fs, n = 2_046_000, 2046
    scene = bench.make_scene(np.random.default_rng(rng_seed), B, 8, fs, 0.010)
    iq = eng.alloc(B * T * n * 8)
    eng.synth_iq(iq, B, T * n, T, scene, 0.05, seed)
    bins = np.arange(-5000, 5000, 500, dtype=np.float64)
    n_units = B * T
    out_dev = eng.alloc(n_units * 32 * len(bins) * CELL.itemsize)
    eng.correlate_grid_dev(iq.ptr.value, n_units, n, 1, ALL_IDS, bins, GYP_NON_COHERENT, out_dev.ptr.value)
    assert eng.debug_get("last_grid_path") == 1        # r06: a launch of this size takes the fused kernel (no folded rows in HBM)
    best_dev = eng.alloc(n_units * 32 * BEST_BIN.itemsize)
    if refined:      # the float64 tie-break between near-equal bins (gyp_grid_best_bins_refined_dev)
        n_ref = eng.grid_best_bins_refined_dev(iq.ptr.value, n_units, n, 1, ALL_IDS, bins, GYP_NON_COHERENT, out_dev.ptr.value, best_dev.ptr.value)
        print(f"[refined best bins] {n_ref} of {n_units * 32} rows had more than one bin within 2e-5 of the row maximum and were decided in float64")
    else:
        eng.grid_best_bins_dev(out_dev.ptr.value, n_units * 32, len(bins), best_dev.ptr.value)
    cells = out_dev.download(CELL, n_units * 32 * len(bins)).reshape(n_units, 32, len(bins))
    best = best_dev.download(BEST_BIN, n_units * 32).reshape(n_units, 32)
    host_iq = iq.download(np.complex64, n_units * n).reshape(n_units, n)
    for b in (iq, out_dev, best_dev):
        b.free()
    return scene, bins, cells, best, host_iq


def _check_rows(eng, cells, best, host_iq, rows, label):
    """`rows` = [(unit, sat_id)]: all 20 cells of each row and its best-bin record against the oracle.  The pool's results are collected
    first and compared afterwards (an assertion inside a live imap loop would have to tear the pool down under load)."""
    fs, n = 2_046_000, 2046
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    path = os.path.join(_shm_dir(), f"gyp_grid_{os.getpid()}.npy")
    np.save(path, host_iq)
    procs = survey_worker.pool_size(max(1, len(rows) // 16))
    per = max(1, -(-len(rows) // (procs * 4)))
    jobs = [(path, fs, n, 1, rows[i:i + per]) for i in range(0, len(rows), per)]
    t0 = time.time()
    try:
        with mp.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(survey_worker.run_grid_rows, jobs, chunksize=1)
    finally:
        os.unlink(path)
    t_pool = time.time() - t0
    tally = {"rows": 0, "cells": 0, "argmax_knife": 0, "bin_knife": 0, "worst_peak": 0.0, "worst_strength": 0.0}
    for rws, bin_idx, peak_index, strength, bmax, bargmax, bstrength, bgap in parts:
        k, nb = bmax.shape
        c = cells[rws[:, 0], rws[:, 1] - 1]                      # [k, bins] device records
        tally["rows"] += k
        tally["cells"] += k * nb
        bad = c["argmax"] != bargmax
        # arg-max: bit-exact, except where the reference's own two largest lags are closer than float32 can tell apart
        assert np.all(bgap[bad] < GAP), (label, rws[bad.any(axis=1)][:3], c["argmax"][bad][:3], bargmax[bad][:3], bgap[bad][:3])
        tally["argmax_knife"] += int(bad.sum())
        rel = np.abs(c["peak"].astype(np.float64) - bmax) / bmax
        tally["worst_peak"] = max(tally["worst_peak"], float(rel.max()))
        assert rel.max() <= 1e-4, (label, rws[np.unravel_index(int(rel.argmax()), rel.shape)[0]], float(rel.max()))
        srel = np.abs(eng.cell_strength(np.ascontiguousarray(c.reshape(-1))).reshape(k, nb) - bstrength) / bstrength
        # (where the reference's top two are closer than float32 resolution the device sees TWO maxima -- n_max = 2 -- and utils.py:111-116
        # leaves both out of the mean: the strength moves by ~(max - mean) / N ~ 1e-3.  Same knife edge as the arg-max: not compared, counted)
        knife = bgap < GAP
        tally["strength_knife"] = tally.get("strength_knife", 0) + int((knife & ~bad).sum())
        srel[knife | bad] = 0.0
        tally["worst_strength"] = max(tally["worst_strength"], float(srel.max()))
        assert srel.max() <= 1e-4, (label, rws[np.unravel_index(int(srel.argmax()), srel.shape)[0]], float(srel.max()))
        # the device's selection (grid_best_bin_kernel, acquisition.py:180-189: the first bin holding the largest maximum)
        g = best[rws[:, 0], rws[:, 1] - 1]
        other = g["bin"] != bin_idx
        if other.any():
            top2 = np.sort(bmax[other], axis=1)[:, -2:]
            assert np.all((top2[:, 1] - top2[:, 0]) / top2[:, 1] < GAP), (label, rws[other][:3], g["bin"][other][:3], bin_idx[other][:3])
            tally["bin_knife"] += int(other.sum())
        ok = ~other & ~(bad | knife)[np.arange(k), bin_idx]
        assert np.array_equal(g["argmax"][ok], peak_index[ok]), (label, rws[ok][g["argmax"][ok] != peak_index[ok]][:3])
        assert np.all(np.abs(g["strength"][ok] - strength[ok]) <= 1e-4 * strength[ok]), label
    print(f"[{label}] {tally['rows']} (unit, satellite) rows = {tally['cells']} cells and {tally['rows']} best-bin records against the oracle (pool of "
          f"{procs} processes: {t_pool:.0f} s; comparison {time.time() - t0 - t_pool:.0f} s): arg-max / best bin bit-exact except {tally['argmax_knife']} cells / "
          f"{tally['bin_knife']} rows where the reference's own top two are < {GAP:g} apart ({tally.get('strength_knife', 0)} more such cells left out of the strength comparison); worst peak difference {tally['worst_peak']:.1e}, worst strength "
          f"difference {tally['worst_strength']:.1e} (bar 1e-4)")
    return tally


def test_cfg2_launch_shape_against_the_oracle(engine_factory):
    """cfg2 as bench.py launches it by default: 128 streams x 64 ms = 8192 units x 640 cells in one gyp_correlate_grid_dev call.  The eight
    planted satellites of 24 units spread over the launch + 1024 random (unit, satellite) rows: 1216 rows = 24 320 cells."""
    fs, n = 2_046_000, 2046
    eng = engine_factory(fs, n)
    B, T = 128, 64
    scene, bins, cells, best, host_iq = _noncoherent_grid(eng, B, T, 99, 5)
    rng = np.random.default_rng(2026)
    rows = []
    for unit in np.linspace(0, B * T - 1, 24).astype(int):
        rows += [(int(unit), int(sv)) for sv in scene[unit // T]["sat_id"]]
    rows += [(int(u), int(s)) for u, s in zip(rng.integers(0, B * T, 1024), rng.integers(1, 33, 1024))]
    t = _check_rows(eng, cells, best, host_iq, rows, "cfg2 launch shape (8192 units x 640 cells)")
    assert t["rows"] == len(rows) and t["argmax_knife"] <= 2 and t["bin_knife"] <= 1
    # the planted satellites are where the scene put them (what bench.py's `*_found` reports), now as a consequence of parity
    found = 0
    for unit in (0, B * T - 1):
        for sat in scene[unit // T]:
            o = cells[unit, int(sat["sat_id"]) - 1]
            b = int(np.argmax(o["peak"]))
            found += int(abs(bins[b] - sat["doppler_hz"]) <= 500 and abs(int(o["argmax"][b]) - int(sat["code_phase"])) <= 1)
    assert found >= 12, found


def test_cfg4_launch_shape_every_best_bin_record_against_the_oracle(engine_factory):
    """cfg4 on one GPU: 64 streams x 64 ms = 4096 units; EVERY (unit, satellite) row -- 131 072 best-bin records, the 24-byte records the
    multi-GPU form all-gathers, and all 2.6 M cells behind them -- against get_best_doppler_shift_estimation in the worker pool."""
    fs, n = 2_046_000, 2046
    eng = engine_factory(fs, n)
    B, T = 64, 64
    scene, bins, cells, best, host_iq = _noncoherent_grid(eng, B, T, 99, 5, refined=True)
    rows = [(u, sv) for u in range(B * T) for sv in ALL_IDS]
    t = _check_rows(eng, cells, best, host_iq, rows, "cfg4 launch shape (64 streams x 64 ms, every record, float64 tie-break between bins)")
    assert t["rows"] == B * T * 32
    assert t["argmax_knife"] <= 8, t       # arg-max WITHIN a cell: expected ~1 per 1e6 cells from the gap statistics; printed above
    assert t["bin_knife"] == 0, t          # the best BIN of all 131 072 rows as the reference picks it: near-equal bins are decided in float64


def test_cfg5_launch_shape_against_the_oracle(engine_factory):
    """cfg5 as bench.run_cfg5 launches it: 4 streams x 32 satellites x range(-10000, 10000, 100) Hz x 10 ms coherent = 25 600 cells in one call
    (48 polyphase branches per unit cut into runs, partial statistics merged by grid_merge_parts_kernel).  Every planted cell (8 per
    stream, at its nearest bin) and its two neighbours + 96 random cells, against integrate_correlation(Coherent) at N = 49 104."""
    import bench

    fs, n = 49_104_000, 49_104
    eng = engine_factory(fs, n)
    n_ms, n_streams = 10, 4
    scene = bench.make_scene(np.random.default_rng(20260925), n_streams, 8, fs, 0.0008)
    scene["doppler_hz"] *= 2.0
    iq = eng.alloc(n_streams * n_ms * n * 8)
    eng.synth_iq(iq, n_streams, n_ms * n, n_ms, scene, 0.005, 555)
    bins = np.arange(-10000, 10000, 100, dtype=np.float64)
    out_dev = eng.alloc(n_streams * 32 * len(bins) * CELL.itemsize)
    eng.correlate_grid_dev(iq.ptr.value, n_streams, n_ms * n, n_ms, ALL_IDS, bins, GYP_COHERENT, out_dev.ptr.value)
    got = out_dev.download(CELL, n_streams * 32 * len(bins)).reshape(n_streams, 32, len(bins))
    host_iq = iq.download(np.complex64, n_streams * n_ms * n).reshape(n_streams, n_ms * n)
    iq.free(); out_dev.free()
    cells, planted = [], []
    for s in range(n_streams):
        for sat in scene[s]:
            b = int(round((min(max(100.0 * round(float(sat["doppler_hz"]) / 100.0), -10000.0), 9900.0) + 10000.0) / 100.0))
            planted.append((s, int(sat["sat_id"]), b, int(sat["code_phase"])))
            for bb in (b - 1, b, b + 1):
                if 0 <= bb < len(bins):
                    cells.append((s, int(sat["sat_id"]), float(bins[bb])))
    rng = np.random.default_rng(55)
    cells += [(int(s), int(sv), float(bins[b])) for s, sv, b in zip(rng.integers(0, n_streams, 96), rng.integers(1, 33, 96), rng.integers(0, len(bins), 96))]
    path = os.path.join(_shm_dir(), f"gyp_cfg5_{os.getpid()}.npy")
    np.save(path, host_iq)
    procs = survey_worker.pool_size(len(cells))
    per = max(1, -(-len(cells) // (procs * 2)))
    t0 = time.time()
    knife, worst_peak, worst_strength, n_done = 0, 0.0, 0.0, 0
    try:
        with mp.get_context("spawn").Pool(procs) as pool:
            for part in pool.imap_unordered(survey_worker.run_coherent_cells, [(path, fs, n, n_ms, cells[i:i + per]) for i in range(0, len(cells), per)]):
                for s, sv, d, argmax, peak, strength, gap, n_max in part:
                    g = got[s, sv - 1, int(round((d + 10000.0) / 100.0))]
                    n_done += 1
                    if int(g["argmax"]) != argmax or gap < GAP:
                        assert gap < GAP, (s, sv, d, int(g["argmax"]), argmax, gap)
                        knife += 1
                        continue
                    assert int(g["n_max"]) == n_max, (s, sv, d)
                    worst_peak = max(worst_peak, abs(float(g["peak"]) - peak) / peak)
                    worst_strength = max(worst_strength, abs(float(eng.cell_strength(np.array([g]))[0]) - strength) / strength)
    finally:
        os.unlink(path)
    print(f"[cfg5 launch shape (4 streams x 32 x 200 x 10 ms coherent)] {n_done} cells against the oracle in {time.time() - t0:.0f} s ({procs} processes): "
          f"arg-max bit-exact except {knife} cells where the reference's own top two are < {GAP:g} apart; worst peak difference {worst_peak:.1e}, "
          f"worst strength difference {worst_strength:.1e} (bar 1e-4)")
    assert n_done == len(cells) and knife <= 1
    assert worst_peak <= 1e-4 and worst_strength <= 1e-4
    hits = sum(int(abs(int(got[s, sv - 1, b]["argmax"]) - cp) <= 1) for s, sv, b, cp in planted)
    assert hits >= 0.8 * len(planted), (hits, len(planted))


@pytest.mark.parametrize("fs,n_ms,integration", [(2_046_000, 1, GYP_NON_COHERENT), (8_184_000, 1, GYP_NON_COHERENT), (2_046_000, 3, GYP_COHERENT),
                                                 (4_092_000, 1, GYP_NON_COHERENT), (1_023_000, 2, GYP_COHERENT)])
def test_fused_grid_kernel_against_folded_rows_and_oracle(engine_factory, fs, n_ms, integration):
    """r06's grid_cells_wave_fused_kernel (the fold inside the cells kernel, every satellite of a (stream, bin) unit on one wavefront)
    against r05's grid_fold_kernel + grid_cells_wave_shared_kernel on the same launch (`no_grid_fused`), and against the oracle on sampled
    cells.  The two stage a row with different summation orders (a direct K-sample sum here, a sliding window there), so magnitudes agree
    to float32 rounding, not bit for bit; an arg-max may differ only between lags whose magnitudes agree to that rounding."""
    import bench
    from oracle import gypsum_oracle as orc

    n = fs // 1000
    eng = engine_factory(fs, n)
    B = 216                                                   # x 20 bins = 4320 units: past the fused path's threshold (16 per CU)
    scene = bench.make_scene(np.random.default_rng(77 + n), B, 6, fs, 20.0 / n)
    iq = eng.alloc(B * n_ms * n * 8)
    eng.synth_iq(iq, B, n_ms * n, n_ms, scene, 6 * 20.0 / n, 4242)
    bins = np.arange(-5000, 5000, 500, dtype=np.float64)
    out_dev = eng.alloc(B * 32 * len(bins) * CELL.itemsize)

    def run():
        eng.correlate_grid_dev(iq.ptr.value, B, n_ms * n, n_ms, ALL_IDS, bins, integration, out_dev.ptr.value)
        return out_dev.download(CELL, B * 32 * len(bins)).reshape(B, 32, len(bins)), int(eng.debug_get("last_grid_path"))

    fused, path = run()
    assert path == 1
    eng.debug_set("grid_fused_waves", 8)      # the 8-wavefront form of the same kernel (replica prefetched into registers): same arithmetic, same bytes
    try:
        fused8, path = run()
    finally:
        eng.debug_set("grid_fused_waves", 12)
    assert path == 1 and fused8.tobytes() == fused.tobytes()
    eng.debug_set("no_grid_fused", 1)
    try:
        rows, path = run()
    finally:
        eng.debug_set("no_grid_fused", 0)
    assert path == 2
    np.testing.assert_allclose(fused["peak"], rows["peak"], rtol=3e-6)
    np.testing.assert_allclose(fused["sum"], rows["sum"], rtol=3e-6)
    other = fused["argmax"] != rows["argmax"]
    assert other.mean() < 1e-4, other.sum()
    assert np.array_equal(fused["n_max"][~other], rows["n_max"][~other]) or (fused["n_max"] != rows["n_max"]).mean() < 1e-4
    # sampled cells against the reference arithmetic: the planted satellites of three streams at every bin
    host = iq.download(np.complex64, B * n_ms * n).reshape(B, n_ms * n)
    chips = orc.generate_ca_codes()
    kind = orc.COHERENT if integration == GYP_COHERENT else orc.NON_COHERENT
    checked = 0
    for b in (0, B // 2, B - 1):
        for sat in scene[b][:3]:
            sv = int(sat["sat_id"])
            for bi in range(0, len(bins), 3):
                ref = np.abs(orc.integrate_correlation(kind, host[b], fs, n, float(bins[bi]), orc.prn_as_complex(chips[sv - 1], n)))
                top2 = np.partition(ref, -2)[-2:]
                if (top2[1] - top2[0]) / top2[1] < GAP:
                    continue
                g = fused[b, sv - 1, bi]
                assert int(g["argmax"]) == int(np.argmax(ref)), (b, sv, bi)
                assert float(g["peak"]) == pytest.approx(ref.max(), rel=1e-4)
                assert float(eng.cell_strength(np.array([g]))[0]) == pytest.approx(orc.peak_strength(ref), rel=1e-4)
                checked += 1
    assert checked >= 50
    iq.free(); out_dev.free()


def test_refined_best_bin_decides_bins_float32_cannot(engine_factory):
    """Two Doppler bins at equal distance from the true Doppler hold the same maximum by construction: 512 noise-free one-satellite units at
    -250 Hz +- up to 5e-4 Hz put the -500 Hz and the 0 Hz bin within ~1e-7 of each other -- below float32 resolution -- and the reference picks
    by its float64 values (acquisition.py:180-182).  gyp_grid_best_bins_refined_dev re-evaluates such bins in float64 from the samples and must
    agree with the oracle in EVERY unit; the float32 selection (gyp_grid_best_bins_dev) is reported beside it."""
    from oracle import gypsum_oracle as orc

    fs, n = 2_046_000, 2046
    eng = engine_factory(fs, n)
    rng = np.random.default_rng(606)
    U = 512
    chips = orc.generate_ca_codes()
    sv = 7
    prn = orc.prn_as_complex(chips[sv - 1], n).real
    t = np.arange(n) / fs
    iq = np.empty((U, n), dtype=np.complex64)
    for u in range(U):
        d = -250.0 + rng.uniform(-5e-4, 5e-4)
        iq[u] = (0.02 * np.roll(prn, int(rng.integers(0, n))) * np.exp(1j * (2 * np.pi * d * t + rng.uniform(0, 2 * np.pi)))).astype(np.complex64)
    bins = np.arange(-5000, 5000, 500, dtype=np.float64)
    dev = eng.alloc(iq.nbytes).upload(iq)
    sats = [sv, 3, 11, 19]
    out_dev = eng.alloc(U * len(sats) * len(bins) * CELL.itemsize)
    eng.correlate_grid_dev(dev.ptr.value, U, n, 1, sats, bins, GYP_NON_COHERENT, out_dev.ptr.value)
    b32, b64 = eng.alloc(U * len(sats) * BEST_BIN.itemsize), eng.alloc(U * len(sats) * BEST_BIN.itemsize)
    eng.grid_best_bins_dev(out_dev.ptr.value, U * len(sats), len(bins), b32.ptr.value)
    n_ref = eng.grid_best_bins_refined_dev(dev.ptr.value, U, n, 1, sats, bins, GYP_NON_COHERENT, out_dev.ptr.value, b64.ptr.value)
    f32 = b32.download(BEST_BIN, U * len(sats)).reshape(U, len(sats))
    f64 = b64.download(BEST_BIN, U * len(sats)).reshape(U, len(sats))
    want = np.array([orc.best_doppler_bin(0.0, 5000.0, iq[u], fs, n, orc.prn_as_complex(chips[sv - 1], n)) for u in range(U)], dtype=object)
    want_bin = np.array([w.bins.index(w.doppler_hz) for w in want])
    assert set(want_bin) == {9, 10}                                  # -500 Hz or 0 Hz, as the float64 values fall
    wrong32 = int(np.sum(f32[:, 0]["bin"] != want_bin))
    assert np.array_equal(f64[:, 0]["bin"], want_bin), np.flatnonzero(f64[:, 0]["bin"] != want_bin)
    assert np.array_equal(f64[:, 0]["argmax"], np.array([w.peak_index for w in want]))
    assert np.all(f64[:, 0]["reserved"] == 1) and n_ref >= U        # every planted row went through the tie-break
    print(f"[refined best bins] {U} units with two bins within ~1e-7: float64 tie-break agrees with the oracle in all of them; the float32 "
          f"selection differs in {wrong32}")
    assert wrong32 > 0                                               # the case is real: float32 alone cannot decide these rows
    for b in (dev, out_dev, b32, b64):
        b.free()
