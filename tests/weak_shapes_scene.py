"""Scenes, parameter rows and shared checks of the weak-signal shape-edge tests (tests/test_weak_shapes_host.py without a GPU,
tests/test_gpu_weak_shapes_*.py on the device): gyp_weak_refine, gyp_weak_measure and gyp_weak_track_block at the shapes at which
their kernels' index arithmetic takes another path -- a ragged last workgroup, the second trip of a strided loop, full LDS rows, a
second workgroup of candidates, more than eight channels, an absolute millisecond above 2^40 -- all at 1.023 Msps (N = 1023).

Everything here is rendered or computed once per process and handed out read-only.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import List, Tuple

import numpy as np

import hybrid_model as hm
import weak_measure_model as mm
import weak_refine_model as rm
import weak_track_model as wm
from gypsum_amd import _lib, _records, engine, synth

N, FS = 1023, 1_023_000
FIRST_MS = 7
BIG_FIRST_MS = 2 ** 40 + 13                 # (2^40 + 13) % 20 = 9: not the 13 a truncation to 32 bits would leave


# ---------------------------------------------------------------------------------------------- record builders and the shared bar
def results_of(rows) -> np.ndarray:
    """WEAK_RESULT records from (stream, sat_id, doppler_hz, carrier_phase, code_phase) rows."""
    out = np.zeros(len(rows), dtype=_lib.WEAK_RESULT)
    for r, (stream, sv, f, phase, cp) in zip(out, rows):
        r["stream"], r["sat_id"], r["doppler_hz"], r["carrier_phase"], r["code_phase"] = stream, sv, f, phase, cp
    return out


def refined_of(rows) -> np.ndarray:
    """WEAK_REFINED records from (stream, sat_id, doppler_hz, carrier_phase, code_phase, edge) rows."""
    out = np.zeros(len(rows), dtype=_lib.WEAK_REFINED)
    for r, (stream, sv, f, phase, cp, edge) in zip(out, rows):
        r["stream"], r["sat_id"], r["doppler_hz"], r["carrier_phase"], r["code_phase"], r["edge"] = stream, sv, f, phase, cp, edge
    return out


def inits_of(records: np.ndarray) -> np.ndarray:
    """CHAN_INIT records from WEAK_RESULT or WEAK_REFINED records."""
    out = np.zeros(len(records), dtype=_lib.CHAN_INIT)
    for name in ("stream", "sat_id", "doppler_hz", "carrier_phase", "code_phase"):      # by field name
        out[name] = records[name]
    return out


def close_to(got: np.ndarray, want: rm.Refined, f0: float, phase0: float) -> None:
    """The tolerances of tests/test_weak_refine_host.py: bin, edge and status equal, delta_hz and carrier_phase within 1e-6, the two
    ratios within 1e-9 relative."""
    assert (int(got["bin"]), int(got["edge"]), int(got["status"])) == (want.bin, want.edge, want.status)
    assert abs(float(got["delta_hz"]) - want.delta_hz) <= 1e-6
    assert abs(float(got["doppler_hz"]) - (f0 + want.delta_hz)) <= 1e-6 + abs(f0) * 2.0 ** -52
    turn = float(got["carrier_phase"]) - rm.wrap_phase(phase0 + want.carrier_phase)
    assert abs(turn - 2 * math.pi * round(turn / (2 * math.pi))) <= 1e-6 and -math.pi < float(got["carrier_phase"]) <= math.pi
    for name, w in (("peak_to_mean", want.peak_to_mean), ("edge_ratio", want.edge_ratio)):
        assert (math.isnan(float(got[name])) and math.isnan(w)) or abs(float(got[name]) - w) <= 1e-9 * abs(w), name


def differences(got: np.ndarray, want: rm.Refined, f0: float, phase0: float) -> Tuple[float, float, float, float]:
    """What close_to bounds, as figures: |delta_hz|, |carrier_phase| (mod 2 pi), and the relative differences of the two ratios (0
    where both are NaN)."""
    turn = float(got["carrier_phase"]) - rm.wrap_phase(phase0 + want.carrier_phase)

    def rel(g: float, w: float) -> float:
        return 0.0 if math.isnan(g) and math.isnan(w) else abs(g - w) / abs(w)

    return (abs(float(got["delta_hz"]) - want.delta_hz), abs(turn - 2 * math.pi * round(turn / (2 * math.pi))),
            rel(float(got["peak_to_mean"]), want.peak_to_mean), rel(float(got["edge_ratio"]), want.edge_ratio))


def as_refined(rec) -> rm.Refined:
    """A WEAK_REFINED record of the host twin (input Doppler and carrier phase 0) as the model's Refined."""
    return rm.Refined(float(rec["delta_hz"]), float(rec["carrier_phase"]), int(rec["edge"]), float(rec["peak_to_mean"]), float(rec["edge_ratio"]),
                      int(rec["bin"]), int(rec["status"]), None, None)


def params_record(p: rm.Params) -> _records.WeakRefineParams:
    return _records.WeakRefineParams(p.span_hz, p.step_hz, p.presum_ms)


def twin_record(prompts: np.ndarray, first_ms: int, p: rm.Params) -> np.ndarray:
    """gyp_weak_refine_estimate on these prompts: the WEAK_REFINED record."""
    return engine.weak_refine_estimate(prompts, first_ms, params_record(p))


def twin(prompts: np.ndarray, first_ms: int, p: rm.Params) -> rm.Refined:
    return as_refined(twin_record(prompts, first_ms, p))


@lru_cache(maxsize=None)
def chips_pm(sat_id: int) -> np.ndarray:
    return mm.chips_pm(sat_id)


# ---------------------------------------------------------------------------------------------- the hand-over's scene and rows
REFINE_SCENE_MS = 2045                      # 2000 for the hand-over, 45 more for the bank behind a SYNC of 2000
#   stream, satellite, the scene's Doppler, carrier phase of the candidate, code phase, bit offset: code phase 0 with +10 kHz, code
#   phase N - 1 with -10 kHz, a carrier phase a hair below zero (the start rule makes its u0 0), and one in the middle
REFINE_SATS = ((0, 5, 10000.0, 0.7, 0, 5), (1, 9, -10000.0, -2.0, N - 1, 10), (0, 17, 1234.5, -1e-300, N // 3, 13), (1, 30, -250.25, 3.0, N // 2 + 1, 0))
# the residual Doppler (scene - candidate) of each candidate: within 0.05 Hz of a multiple of 0.5 Hz, because at 2000 ms the main
# lobe is 0.5 Hz from null to null and the 0.5-Hz grid would otherwise sample it near its nulls
RESIDUALS = (-3.05, 4.05, 6.45, -1.55)
END_RESIDUALS = (8.3, -8.3, 8.3, -8.3)      # beyond a span of 5 Hz: the first sidelobe (3.3 Hz from the peak at 223 ms) tops at the end bin

DEFAULTS = rm.Params()
#              n_ms  params                          G     J     guard  residuals
REFINE_ROWS = ((41, DEFAULTS, 10, 40, 49, RESIDUALS),                              # n_ms % 4 = 1, 2, 3: the sums kernel's ragged last workgroup
               (42, DEFAULTS, 10, 40, 48, RESIDUALS),
               (43, DEFAULTS, 10, 40, 47, RESIDUALS),
               (223, DEFAULTS, 55, 40, 9, RESIDUALS),                              # guard 9: a finite peak_to_mean; a tail of 3 ms
               (223, rm.Params(20.0, 0.5, 5), 44, 40, 9, RESIDUALS),               # another presum and tail
               (223, rm.Params(12.0, 1.0, 20), 11, 12, 5, RESIDUALS),              # the presum of twenty
               (257, rm.Params(20.0, 0.5, 1), 257, 40, 8, RESIDUALS),              # the second trip of the n_ms and G loops
               (2000, rm.Params(20.0, 0.5, 1), 2000, 40, 1, RESIDUALS),            # G = 2000: every LDS row full
               (2000, rm.Params(64.0, 0.03125, 2), 1000, 2048, 16, RESIDUALS),     # J = 2048 exactly: 4097 bins
               (223, rm.Params(5.0, 0.5, 4), 55, 10, 9, END_RESIDUALS))            # the end bin: status 1
REFINE_IDS = [f"{n_ms}ms-span{p.span_hz:g}-step{p.step_hz:g}-presum{p.presum_ms}" for n_ms, p, *_ in REFINE_ROWS]
MODEL_LIMIT = 10 ** 6                       # rm.estimate walks n_bins * G terms in a Python loop: beyond this it takes minutes


def is_end_row(row) -> bool:
    return row[5] is END_RESIDUALS


def within_model(row) -> bool:
    n_ms, p = row[0], row[1]
    _, G, J, _ = rm.shape(p, n_ms)
    return (2 * J + 1) * G <= MODEL_LIMIT


def refine_true_edge(i: int, first_ms: int = FIRST_MS) -> int:
    """Millisecond m of the scene starts a bit of candidate i when (m + bit offset) % 20 == 0; the buffer begins at the scene's first
    millisecond, which is the absolute millisecond first_ms."""
    return (first_ms - REFINE_SATS[i][5]) % 20


@lru_cache(maxsize=None)
def refine_iq() -> np.ndarray:
    """complex64[2, REFINE_SCENE_MS * N], read-only: two strong satellites a stream, code Doppler, the data bits change every 20 ms."""
    a, sigma = synth.default_amplitudes(FS)
    rng = np.random.default_rng([20261021, 0x5A7E])
    streams = []
    for s in (0, 1):
        sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=f, code_phase=cp, carrier_phase=float(rng.uniform(-np.pi, np.pi)), amplitude=a,
                                         nav_bits=np.array([1, -1, 1, -1], dtype=np.int8), nav_bit_offset_ms=off)
                for stream, sv, f, _, cp, off in REFINE_SATS if stream == s]
        streams.append(hm.render(synth.SyntheticScene(fs=FS, n_ms=REFINE_SCENE_MS, sats=sats, noise_sigma=sigma, seed=700 + s), code_doppler=True))
    x = np.ascontiguousarray(np.stack(streams), dtype=np.complex64)
    x.setflags(write=False)
    return x


def head_of(x: np.ndarray, n_ms: int, start_ms: int = 0) -> np.ndarray:
    """Milliseconds start_ms .. start_ms + n_ms of every stream, contiguous."""
    return np.ascontiguousarray(x[:, start_ms * N:(start_ms + n_ms) * N])


def refine_results(residuals=RESIDUALS) -> np.ndarray:
    """The four candidates, each `residual` below the scene's Doppler."""
    out = results_of([(stream, sv, f - res, phase, cp) for (stream, sv, f, phase, cp, _), res in zip(REFINE_SATS, residuals)])
    out.setflags(write=False)
    return out


_model_sums = {}


def model_sums(residuals, n_ms: int) -> np.ndarray:
    """rm.open_loop_sums of the four candidates over the scene's first n_ms milliseconds, complex128[4, n_ms].  Open loop: a shorter
    buffer's sums are the head of a longer one's, so each set of residuals is computed once at its longest."""
    have = _model_sums.get(residuals)
    if have is None:
        x = refine_iq()
        res = refine_results(residuals)
        longest = max(row[0] for row in REFINE_ROWS if row[5] is residuals)
        have = np.stack([rm.open_loop_sums(x[int(r["stream"])], chips_pm(int(r["sat_id"])), FS, N, float(r["doppler_hz"]), float(r["carrier_phase"]),
                                           int(r["code_phase"]), longest) for r in res])
        have.setflags(write=False)
        _model_sums[residuals] = have
    return have[:, :n_ms]


def model_prompts(residuals, n_ms: int) -> np.ndarray:
    return model_sums(residuals, n_ms).astype(np.complex64)


def peak_margin(prompts: np.ndarray, p: rm.Params, k: int) -> float:
    """min over the neighbours of bin k of P[k] / P[neighbour], the three bins evaluated with rm.sum_at."""
    L, G, J, _ = rm.shape(p, len(prompts))
    sr, si = rm.squares(prompts, L, G)

    def power(j: int) -> float:
        yr, yi = rm.sum_at(sr, si, L, float(j - J) * p.step_hz)
        return yr * yr + yi * yi

    return min(power(k) / power(j) for j in (k - 1, k + 1) if 0 <= j <= 2 * J)


# ---------------------------------------------------------------------------------------------- the measurement's scene and rows
MEASURE_SCENE_MS = 2001
#   stream, satellite, Doppler, carrier phase of the candidate, integer code phase, the fraction added to it in the scene.  Every
#   satellite's bits change at the scene's milliseconds 0, 20, 40, ...: a buffer that begins at the scene's millisecond s has its
#   first bit edge at index (-s) % 20, so the start picks the head.  Over the first 19 ms the code drifts 0.13 samples at most: the
#   integer code phases hold for every start used here.
MEASURE_SATS = ((0, 5, 10000.0, 0.7, 0, 0.31), (1, 9, -10000.0, -2.0, N - 1, -0.42), (0, 17, 1234.5, -1e-300, N // 3, 0.18), (1, 30, -250.25, 3.0, N // 2 + 1, -0.07))
#               n_ms  start  head  groups
MEASURE_ROWS = ((41, 7, 13, 1),             # n_ms % 4 = 1, 2, 3
                (42, 0, 0, 2),
                (43, 19, 1, 2),
                (59, 1, 19, 2),             # two groups and no spare millisecond
                (60, 19, 1, 2),             # two groups and 19 spare milliseconds
                (2000, 0, 0, 100),          # every thread of the fold kernel that can have a group has one
                (2000, 1, 19, 99))
MEASURE_IDS = [f"{n_ms}ms-head{head}" for n_ms, _, head, _ in MEASURE_ROWS]
#          passes  spacing        (tests/test_gpu_weak_measure.py's)
SETTINGS = ((2, 1 << 39), (4, 1 << 36), (1, 1 << 38))
SIX = ("minus_re", "minus_im", "prompt_re", "prompt_im", "plus_re", "plus_im")


def measure_edge(head: int, first_ms: int = FIRST_MS) -> int:
    """The edge for which the first group's head is `head` in a buffer whose first millisecond is first_ms."""
    return (first_ms + head) % 20


@lru_cache(maxsize=None)
def measure_iq() -> np.ndarray:
    """complex64[2, MEASURE_SCENE_MS * N], read-only: the satellites at fractional code phases."""
    a, sigma = synth.default_amplitudes(FS)
    rng = np.random.default_rng([20261021, 0x3EA5])
    streams = []
    for s in (0, 1):
        sats = [mm.Sat(sv, f, cp + frac, float(rng.uniform(-np.pi, np.pi)), a, np.array([1, -1, 1, -1], dtype=np.int8), 0)
                for stream, sv, f, _, cp, frac in MEASURE_SATS if stream == s]
        streams.append(mm.render(sats, FS, N, MEASURE_SCENE_MS, sigma, 900 + s))
    x = np.ascontiguousarray(np.stack(streams), dtype=np.complex64)
    x.setflags(write=False)
    return x


def measure_refined(head: int, first_ms: int = FIRST_MS) -> np.ndarray:
    out = refined_of([(stream, sv, f, phase, cp, measure_edge(head, first_ms)) for stream, sv, f, phase, cp, _ in MEASURE_SATS])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- many candidates
def many_results(count: int) -> np.ndarray:
    """`count` WEAK_RESULT records cycling the four kinds over the two streams, every one with its own Doppler and the satellites 1..32
    in turn; the first four are the scene's candidates."""
    rows = []
    for i in range(count):
        stream, _, f, phase, cp, _ = REFINE_SATS[i % 4]
        base = refine_results()[i % 4]
        rows.append((stream, int(base["sat_id"]) if i < 4 else 1 + (7 * i) % 32, float(base["doppler_hz"]) + 12.5 * (i // 4), phase, cp))
    return results_of(rows)


def many_refined(count: int, first_ms: int = FIRST_MS) -> np.ndarray:
    """The same as WEAK_REFINED records, the edges running through 0..19."""
    res = many_results(count)
    return refined_of([(int(r["stream"]), int(r["sat_id"]), float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["code_phase"]), (3 * i) % 20)
                       for i, r in enumerate(res)])


# ---------------------------------------------------------------------------------------------- the bank
SYNC_MS = (40, 47, 61, 2000)
BANK_FIRST_MS = (0, 7, BIG_FIRST_MS)
BANK_AFTER_MS = 45                          # milliseconds behind SYNC in the one call
SPLIT_47 = (1, 46, 1, 19, 25)               # the same 92 ms in five calls
BANK_SIZES = (8, 9, 13, 17)                 # n >> 3 and n & 7 of the workgroup-to-channel map: (1, 0), (1, 1), (1, 5), (2, 1)


def bank_inits(count: int) -> np.ndarray:
    """`count` CHAN_INIT records: the scene's candidates in turn, each turn 9 Hz further off, over the two streams."""
    return inits_of(many_results_for_bank(count))


def many_results_for_bank(count: int) -> np.ndarray:
    rows = []
    for i in range(count):
        base = refine_results()[i % 4]
        rows.append((int(base["stream"]), int(base["sat_id"]), float(base["doppler_hz"]) + 9.0 * (i // 4), float(base["carrier_phase"]), int(base["code_phase"])))
    return results_of(rows)


def expected_phases(first_ms: int, sync_ms: int, edge: int, n_ms: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """(phase[n_ms], pos[n_ms], index of the first TRACK millisecond) of a channel created at first_ms that picked `edge`."""
    start = next(i for i in range(sync_ms, sync_ms + 20) if (first_ms + i) % 20 == edge)
    idx = np.arange(n_ms)
    phase = np.where(idx < sync_ms, wm.SYNC, np.where(idx < start, wm.WAIT, wm.TRACK))
    pos = np.where(idx < start, 0, (idx - start) % 20)
    return phase, pos, start
