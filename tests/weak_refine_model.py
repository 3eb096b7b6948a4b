"""numpy float64 model of the weak-signal hand-over (include/gypsum_hip.h, "weak-signal hand-over"): steps 2-7 restated from the
header on given prompts, the open-loop prompts of step 1 from tests/weak_track_model.py, and the refusals.

The sums walk g (and j, for the quality figure) in the header's order with one IEEE rounding per operation; the sine and cosine are
numpy's, so the library's host form agrees to about 1e-12 in delta_hz and carrier_phase, not bit for bit.

`python tests/weak_refine_model.py <seed> ...` prints what tests/test_weak_refine_host.py gates on the closed-loop scene of
tests/weak_track_scene.py, for each satellite of FAR_BIN_STARTS from the search's farther fine bin, carrier phase 0.3, the first 220 ms:
the refined Doppler against the truth at the true code phase and one sample off, the edge, the carrier phase against the scene's
(mod pi), peak_to_mean, and the model's tracker from the refined start.  tests/test_weak_refine_host.py records the figures of
seeds 99 and 322 in its docstring: refined errors of 0.01 to 0.24 Hz from starts 7 and 8 Hz off (up to 0.35 Hz one sample off the
code phase), the true edge on all six, the carrier phase within 0.22 rad, peak_to_mean 32 to 49 (5.7 to 13.2 one sample off).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

import weak_track_model as wm

MIN_MS, MAX_MS, MIN_GROUPS, MAX_BINS = 40, 2000, 8, 4097
PRESUMS = (1, 2, 4, 5, 10, 20)
TWO_PI = 6.283185307179586476925


@dataclass
class Params:
    span_hz: float = 20.0
    step_hz: float = 0.5
    presum_ms: int = 4


@dataclass
class Refined:
    delta_hz: float
    carrier_phase: float      # the increment: add the input's and wrap for the record's
    edge: int
    peak_to_mean: float
    edge_ratio: float
    bin: int
    status: int
    power: np.ndarray         # P_j, j = -J..J
    energies: np.ndarray      # en[20] of the derotated prompts


def refusal(p: Params, n_ms: int, first_ms: int) -> Optional[str]:
    """refine_refusal: why a request is refused, in the header's order."""
    if not 0.0 < p.span_hz <= 100.0:
        return "span_hz must be in (0, 100]"
    if not 0.01 <= p.step_hz <= p.span_hz:
        return "step_hz must be in [0.01, span_hz]"
    if p.presum_ms not in PRESUMS:
        return "presum_ms must be one of 1, 2, 4, 5, 10, 20"
    if p.span_hz >= 250.0 / p.presum_ms:
        return "span_hz must be below 250 / presum_ms"
    if math.floor(p.span_hz / p.step_hz) > (MAX_BINS - 1) // 2:
        return "more than 4097 bins"
    if not MIN_MS <= n_ms <= MAX_MS:
        return "n_ms must be 40..2000"
    if n_ms // p.presum_ms < MIN_GROUPS:
        return "fewer than 8 groups of presum_ms milliseconds"
    if first_ms < 0:
        return "first_ms is negative"
    return None


def shape(p: Params, n_ms: int) -> Tuple[int, int, int, int]:
    """(L, G, J, guard)."""
    return p.presum_ms, n_ms // p.presum_ms, int(math.floor(p.span_hz / p.step_hz)), int(math.ceil(1000.0 / (float(n_ms) * p.step_hz)))


def rotor(cycles):
    """exp(-2 pi i c), c reduced by rint(c) first (scalar or array)."""
    c = np.asarray(cycles, dtype=np.float64)
    a = -TWO_PI * (c - np.rint(c))
    return np.cos(a), np.sin(a)


def squares(prompts: np.ndarray, L: int, G: int) -> Tuple[np.ndarray, np.ndarray]:
    p = np.asarray(prompts, dtype=np.complex64)
    qr, qi = np.zeros(G), np.zeros(G)
    for i in range(L):                              # in order
        qr = qr + p.real[i:G * L:L].astype(np.float64)
        qi = qi + p.imag[i:G * L:L].astype(np.float64)
    return qr * qr - qi * qi, (2.0 * qr) * qi


def group_times(L: int, G: int) -> np.ndarray:
    return (np.arange(G, dtype=np.float64) * L + 0.5 * L) / 1000.0


def sum_at(sr: np.ndarray, si: np.ndarray, L: int, f_hz: float) -> Tuple[float, float]:
    """Y(f): the terms in numpy, added in increasing g one by one."""
    wr, wi = rotor((2.0 * np.float64(f_hz)) * group_times(L, len(sr)))
    tr, ti = sr * wr - si * wi, sr * wi + si * wr
    ar = ai = 0.0
    for a, b in zip(tr.tolist(), ti.tolist()):
        ar += a
        ai += b
    return ar, ai


def wrap_phase(x: float) -> float:
    """x wrapped to (-pi, pi]."""
    return x - TWO_PI * math.ceil((x - math.pi) / TWO_PI)


def pick(P: np.ndarray, J: int, step_hz: float, guard: int) -> Tuple[int, int, float, float]:
    """(bin, status, delta_hz, peak_to_mean)."""
    k = int(np.argmax(P))                           # the lowest index on a tie
    if not P[k] > 0.0:
        return J, 1, 0.0, float("nan")
    d = 0.0
    at_end = k in (0, len(P) - 1)
    if not at_end:
        den = float(P[k - 1]) - 2.0 * float(P[k]) + float(P[k + 1])
        if den < 0.0:
            d = min(0.5, max(-0.5, 0.5 * (float(P[k - 1]) - float(P[k + 1])) / den))
    far = [float(P[j]) for j in range(len(P)) if abs(j - k) > guard]
    total = 0.0
    for v in far:
        total += v
    with np.errstate(divide="ignore", invalid="ignore"):
        ptm = float(np.float64(P[k]) / (np.float64(total) / np.float64(len(far)))) if far else float("nan")
    return k, int(at_end), (float(k - J) + d) * step_hz, ptm


def derotate(prompts: np.ndarray, delta_hz: float) -> np.ndarray:
    p = np.asarray(prompts, dtype=np.complex64)
    t = (np.arange(len(p), dtype=np.float64) + 0.5) / 1000.0
    wr, wi = rotor(np.float64(delta_hz) * t)
    pr, pi = p.real.astype(np.float64), p.imag.astype(np.float64)
    out = np.empty(len(p), dtype=np.complex64)
    out.real = (pr * wr - pi * wi).astype(np.float32)
    out.imag = (pr * wi + pi * wr).astype(np.float32)
    return out


def estimate(prompts: np.ndarray, first_ms: int, p: Params = Params()) -> Refined:
    """Steps 2-7 on complex64 prompts, the prompt of millisecond first_ms + i at i; input Doppler and carrier phase 0."""
    n_ms = len(prompts)
    assert refusal(p, n_ms, first_ms) is None
    L, G, J, guard = shape(p, n_ms)
    sr, si = squares(prompts, L, G)
    P = np.zeros(2 * J + 1)
    for j in range(-J, J + 1):
        yr, yi = sum_at(sr, si, L, float(j) * p.step_hz)
        P[j + J] = yr * yr + yi * yi
    k, status, delta, ptm = pick(P, J, p.step_hz, guard)
    yr, yi = sum_at(sr, si, L, delta)
    en, edge = wm.bit_sync(derotate(prompts, delta), first_ms)
    order = np.sort(en)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(order[-1]) / np.float64(order[-2]))
    return Refined(delta, wrap_phase(0.5 * math.atan2(yi, yr)), edge, ptm, ratio, k, status, P, en)


def open_loop_sums(x: np.ndarray, chips_pm: np.ndarray, fs: int, n: int, doppler_hz: float, carrier_phase: float, code_phase: int,
                   n_ms: int) -> np.ndarray:
    """Step 1 on the float64 model: the prompt sums a weak bank started from this result would form in SYNC over the first n_ms
    milliseconds of x, complex128 (the device's float32 prompts agree to the project's 1e-4 ||x_ms||_2 bar)."""
    u0, c0 = wm.init_u0(carrier_phase), wm.init_c0(code_phase, n)
    r = wm.code_rate(doppler_hz, n)
    out = np.zeros(n_ms, dtype=np.complex128)
    for m in range(n_ms):
        out[m] = wm.ms_sums(x[m * n:(m + 1) * n], chips_pm, fs, u0, doppler_hz, 0, c0, r, wm.ONE // 2)[1]
        u0, c0 = wm.advance(u0, c0, doppler_hz, fs, n, r)
    return out


def open_loop_prompts(x: np.ndarray, chips_pm: np.ndarray, fs: int, n: int, doppler_hz: float, carrier_phase: float, code_phase: int,
                      n_ms: int) -> np.ndarray:
    """The same rounded to complex64, as the bank keeps them."""
    return open_loop_sums(x, chips_pm, fs, n, doppler_hz, carrier_phase, code_phase, n_ms).astype(np.complex64)


def refine(x: np.ndarray, chips_pm: np.ndarray, fs: int, n: int, doppler_hz: float, carrier_phase: float, code_phase: int, n_ms: int,
           first_ms: int = 0, p: Params = Params()) -> Tuple[float, float, Refined]:
    """(refined Doppler, refined carrier phase, the estimate) of one candidate."""
    est = estimate(open_loop_prompts(x, chips_pm, fs, n, doppler_hz, carrier_phase, code_phase, n_ms), first_ms, p)
    return doppler_hz + est.delta_hz, wrap_phase(carrier_phase + est.carrier_phase), est


SCENE_MS = 220
START_PHASE = 0.3


def scene_rows(seed: int) -> List[dict]:
    """Each FAR_BIN_STARTS start of tests/weak_track_scene.py refined on the scene's first 220 ms, and tracked from there."""
    import weak_track_scene as ws
    tr, x = ws.truth(seed), ws.iq(seed)
    rows = []
    for sv, f in ws.FAR_BIN_STARTS:
        sat = tr[sv]
        f1, ph1, est = refine(x, ws.chips_pm(sv), ws.FS, ws.N, f, START_PHASE, sat.code_phase, SCENE_MS)
        f_off, _, est_off = refine(x, ws.chips_pm(sv), ws.FS, ws.N, f, START_PHASE, (sat.code_phase + 1) % ws.N, SCENE_MS)
        ch, per = ws.track_from(seed, sv, f1, ph1, sat.code_phase)
        phase_err = (ph1 - sat.carrier_phase + math.pi / 2) % math.pi - math.pi / 2
        rows.append(dict(seed=seed, sat=sv, start=f - sat.doppler_hz, error=f1 - sat.doppler_hz, error_off=f_off - sat.doppler_hz, edge=est.edge,
                         true_edge=ws.true_edge(sat), phase_error=phase_err, peak_to_mean=est.peak_to_mean, peak_to_mean_off=est_off.peak_to_mean,
                         edge_ratio=est.edge_ratio, status=est.status, wrong_bits=ws.wrong_bits(sat, per), n_bits=len(per) - ws.SETTLE_PERIODS,
                         phase_rms=ws.phase_rms(per), tracked_edge=ch.edge))
    return rows


def report(seed: int) -> None:
    for r in scene_rows(seed):
        print(f"seed {r['seed']} sat {r['sat']}: start {r['start']:+.0f} Hz -> refined {r['error']:+.3f} Hz off (one sample off: {r['error_off']:+.3f}), "
              f"edge {r['edge']} (true {r['true_edge']}), phase {r['phase_error']:+.3f} rad mod pi, peak/mean {r['peak_to_mean']:.1f} "
              f"(one sample off: {r['peak_to_mean_off']:.1f}), edge ratio {r['edge_ratio']:.2f}, status {r['status']}; tracked from there: "
              f"wrong bits {r['wrong_bits']} of {r['n_bits']}, phase rms {r['phase_rms']:.3f}, edge {r['tracked_edge']}")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
    for a in sys.argv[1:] or ["99"]:
        report(int(a))
