"""numpy float64 model of the hybrid coherent/non-coherent search (include/gypsum_hip.h, "weak-signal acquisition").

`hybrid_cell` is built on `oracle.integrate_correlation(COHERENT, ...)` per block; the rotation, the sets and the statistics
restate section "weak-signal acquisition" of the header; `acquire_weak` runs the two levels; `render` is `synth.render` with the
code time taken at (n - cp) (1 + d / 1575.42e6) and each chip sampled at its sample's centre (its docstring says why), so that a
peak really drifts with the carrier Doppler.

numpy's float64 *, /, -, sqrt are single IEEE roundings and never contracted, which is what hybrid_plan.hpp's hybrid_shift and
hybrid_z do with contraction off: `shift` and `stats` are bit-for-bit models of gyp_hybrid_shift and gyp_hybrid_stats.  The
profiles themselves are float64 here and float32 transforms on the device: records agree to the project's 1e-4 bar, not bitwise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import gypsum_oracle as orc

ALTERNATE, CODE_DOPPLER = 1, 2
L1_HZ = 1575420000.0


def shift(n: int, coherent_ms: int, block: int, doppler_hz: float, flags: int) -> int:
    """gyp_hybrid_shift: llround((double)(b T N) * f / 1575420000.0), half away from zero; 0 without CODE_DOPPLER."""
    if not flags & CODE_DOPPLER:
        return 0
    q = float(np.float64(float(block * coherent_ms * n)) * np.float64(doppler_hz) / np.float64(L1_HZ))
    whole = math.floor(abs(q))                                      # (floor(|q| + 0.5) is wrong just below a half: the sum rounds up)
    return (whole + (1 if abs(q) - whole >= 0.5 else 0)) * (1 if q >= 0 else -1)    # |q| - floor|q| is exact


def z_of(peak: float, n_off: int, sum_off: float, sumsq_off: float) -> float:
    """hybrid_z: population variance, NaN where not defined.  `peak` is the float32 record value (or any float)."""
    if n_off <= 0:
        return float("nan")
    nn = np.float64(n_off)
    mean = np.float64(sum_off) / nn
    m2 = np.float64(sumsq_off) / nn
    var = m2 - mean * mean
    if not var > 0.0:
        return float("nan")
    return float((np.float64(peak) - mean) / np.sqrt(var))


def stats(rec) -> Tuple[float, float]:
    """gyp_hybrid_stats of one HYBRID_CELL-like record (mapping with peak, second, n_off, sum_off, sumsq_off)."""
    z = z_of(float(rec["peak"]), int(rec["n_off"]), float(rec["sum_off"]), float(rec["sumsq_off"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(rec["peak"]) / np.float64(rec["second"]))
    return z, ratio


def block_profiles(iq: np.ndarray, fs: int, n: int, sat: int, f: float, T: int, M: int, replicas: Optional[Dict[int, np.ndarray]] = None) -> np.ndarray:
    """C_b for b < M: complex128[M, n].  Block b is given to the oracle as its whole buffer (time starts at its first sample)."""
    rep = replicas[sat] if replicas is not None else orc.prn_as_complex(orc.generate_ca_codes()[sat - 1], n)
    x = np.asarray(iq).astype(np.complex128)
    return np.stack([orc.integrate_correlation(orc.COHERENT, x[b * T * n:(b + 1) * T * n], fs, n, f, rep) for b in range(M)])


def block_profiles_shared(iq: np.ndarray, fs: int, n: int, sats: Sequence[int], f: float, T: int, M: int,
                          conj_spectra: Optional[np.ndarray] = None) -> np.ndarray:
    """The same C_b for several satellites at one bin, complex128[len(sats), M, n], with the work they share done once: the sum over
    a block's milliseconds commutes with the (linear) correlation, so the wiped milliseconds are folded first and transformed once
    per block -- sum_i ifft(fft(w_i) conj(fft p)) = ifft(fft(sum_i w_i) conj(fft p)).  Equal to block_profiles to float64 rounding
    (tests/test_hybrid_host.py checks it); the searches over thousands of cells use this form."""
    if conj_spectra is None:
        conj_spectra = replica_conj_spectra(n, sats)
    x = np.asarray(iq[:M * T * n]).astype(np.complex128).reshape(M, T * n)
    t = np.arange(T * n) / fs                                     # utils.py:92-96 per millisecond i: arange(N)/fs + (i N)/fs
    folded = (x * np.exp(-1j * orc.TAU * f * t)).reshape(M, T, n).sum(axis=1)
    return np.fft.ifft(np.fft.fft(folded, axis=1)[None, :, :] * conj_spectra[:, None, :], axis=2)


def replica_conj_spectra(n: int, sats: Sequence[int]) -> np.ndarray:
    codes = orc.generate_ca_codes()
    return np.conj(np.fft.fft(np.stack([orc.prn_as_complex(codes[s - 1], n) for s in sats]), axis=1))


@dataclass
class SetStats:
    peak: float
    argmax: int
    second: float
    second_argmax: int
    n_off: int
    sum_off: float
    sumsq_off: float
    z: float
    rival_gap: float          # (peak - largest other value) / peak: np.argmax's own margin
    second_gap: float         # the same for the second peak among the lags away


def set_stats(P: np.ndarray, n: int) -> SetStats:
    spc = n // 1023
    a = int(np.argmax(P))
    peak = float(P[a])
    l = np.arange(n)
    d = np.abs(l - a)
    d = np.minimum(d, n - d)
    away = d > spc
    n_off = int(away.sum())
    others = np.delete(P, a)
    rival_gap = float((peak - others.max()) / peak) if peak > 0 and others.size else 1.0
    if n_off:
        Pa = np.where(away, P, -np.inf)
        sa = int(np.argmax(Pa))
        second = float(P[sa])
        rest = Pa.copy()
        rest[sa] = -np.inf
        second_gap = float((second - rest.max()) / second) if second > 0 and n_off > 1 else 1.0
        sum_off = float(P[away].sum())
        sumsq_off = float((P[away] ** 2).sum())
    else:
        sa, second, second_gap, sum_off, sumsq_off = -1, 0.0, 1.0, 0.0, 0.0
    return SetStats(peak, a, second, sa, n_off, sum_off, sumsq_off, z_of(peak, n_off, sum_off, sumsq_off), rival_gap, second_gap)


@dataclass
class HybridCell:
    set: int
    blocks_used: int
    sets: List[SetStats]
    C0: np.ndarray            # block 0's coherent profile (the carrier phase is its angle at the code phase)

    @property
    def rec(self) -> SetStats:
        return self.sets[self.set]

    @property
    def z(self) -> float:
        return self.rec.z

    @property
    def peak_ratio(self) -> float:
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(self.rec.peak) / np.float64(self.rec.second))


def hybrid_cell(iq: np.ndarray, fs: int, n: int, sat: int, f: float, T: int, M: int, flags: int,
                replicas: Optional[Dict[int, np.ndarray]] = None, profiles: Optional[np.ndarray] = None) -> HybridCell:
    """The record of one (stream, satellite, bin) cell, float64.  `profiles`: block_profiles(...) computed already."""
    if not 1 <= T <= 20 or M < 1 or M * T > 65535 or flags & ~3 or (flags & ALTERNATE and M < 2):
        raise ValueError("refused")
    Cb = profiles if profiles is not None else block_profiles(iq, fs, n, sat, f, T, M, replicas)
    n_sets = 2 if flags & ALTERNATE else 1
    P = np.zeros((n_sets, n))
    for b in range(M):
        pw = Cb[b].real ** 2 + Cb[b].imag ** 2
        P[b & 1 if n_sets == 2 else 0] += np.roll(pw, shift(n, T, b, f, flags))     # P[l] += pw[(l - delta) mod n]
    sets = [set_stats(P[k], n) for k in range(n_sets)]
    pick = 1 if n_sets == 2 and sets[1].z > sets[0].z else 0
    used = M if n_sets == 1 else ((M + 1) // 2 if pick == 0 else M // 2)
    return HybridCell(pick, used, sets, Cb[0])


def coarse_bins(center: float, spread: float, T: int) -> List[float]:
    out, i = [], 0
    while center - spread + i * (500.0 / T) < center + spread:
        out.append(center - spread + i * (500.0 / T))
        i += 1
    return out


def fine_bins(best: float, step: float, T: int) -> List[float]:
    if not step > 0:
        return []
    J = 0
    while (J + 1) * step <= 250.0 / T:
        J += 1
    return [best + float(j) * step for j in range(-J, J + 1)]


def n_coarse(center: float, spread: float, T: int) -> int:
    """hybrid_coarse_bins: len(coarse_bins(...)), with the loop's cap of 1,000,000 (the bins are monotone in i, so the count of a
    prefix is the position of the first bin that is not below center + spread)."""
    i = np.arange(1_000_000, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        below = np.float64(center) - np.float64(spread) + i * (np.float64(500.0) / np.float64(T)) < np.float64(center) + np.float64(spread)
    return len(below) if below.all() else int(np.argmin(below))


def fine_half(step: float, T: int) -> int:
    """hybrid_fine_half: J of fine_bins, with the loop's cap of 500,000; -1 where there is no fine level."""
    if not step > 0:
        return -1
    j = np.arange(1, 500_001, dtype=np.float64)
    with np.errstate(over="ignore"):
        within = j * np.float64(step) <= np.float64(250.0) / np.float64(T)
    return len(within) if within.all() else int(np.argmin(within))


def refusal(T: int, M: int, flags: int) -> Optional[str]:
    """hybrid_refusal: why a request is refused, in the header's order."""
    if not 1 <= T <= 20:
        return "coherent_ms must be 1..20"
    if M < 1:
        return "n_blocks must be at least 1"
    if M * T > 65535:
        return "n_blocks * coherent_ms must be at most 65535"
    if flags & ~3:
        return "unknown flag bits"
    if flags & ALTERNATE and M < 2:
        return "GYP_HYB_ALTERNATE needs at least 2 blocks"
    return None


PLAN_FIELDS = ("fits", "n_sets", "chunk_cells", "n_chunks", "profile", "power", "acc_x")


def plan(n: int, n_cells: int, T: int, M: int, flags: int, scratch_mb: int) -> Tuple[int, ...]:
    """hybrid_plan, the chunk rule restated: a cell holds a float2 profile row and n_sets float power rows of n samples; a chunk has
    as many cells as fit the budget, at least 1, at most 65535 (the accumulate kernel's grid.y) and no more than there are."""
    if refusal(T, M, flags) or not 1 <= n_cells <= 2 ** 31 - 1 or n < 1:
        return (0,) * len(PLAN_FIELDS)
    n_sets = 2 if flags & ALTERNATE else 1
    room = max(1, (scratch_mb << 20) // (n * (8 + 4 * n_sets)))
    chunk = min(n_cells, room, 65535)
    return (1, n_sets, chunk, -(-n_cells // chunk), chunk * n, chunk * n * n_sets, -(-n // 256))


SEARCH_FIELDS = ("n_coarse", "fine_half", "n_fine", "n_states", "coarse_cells", "fine_cells", "level_cells", "records") + tuple("run_" + f for f in PLAN_FIELDS)


def weak_search_plan(n: int, n_streams: int, n_sats: int, T: int, M: int, flags: int, center: float, spread: float, step: float,
                     scratch_mb: int) -> Tuple[Optional[str], Tuple[int, ...]]:
    """gyp_acquire_weak_dev's arithmetic behind its pointer and satellite-id checks, as it stood inline: (why it is refused or None,
    SEARCH_FIELDS -- all 0 when refused)."""
    none = (0,) * len(SEARCH_FIELDS)
    why = refusal(T, M, flags)
    if why:
        return why, none
    if n_sats > 32:
        return "at most 32 satellites per call", none
    if not (math.isfinite(center) and math.isfinite(spread) and math.isfinite(step)) or not spread > 0.0:
        return "center, spread and fine step must be finite and the spread positive", none
    coarse, half = n_coarse(center, spread, T), fine_half(step, T)
    fine = 2 * half + 1 if half >= 0 else 0
    if coarse < 1 or coarse > 4096 or fine > 4096:
        return "a level must have between 1 and 4096 Doppler bins", none
    states = n_streams * n_sats
    if states * max(coarse, fine) > 2 ** 31 - 1:
        return "more than 2^31 - 1 cells", none
    cc, fc = states * coarse, states * fine
    return None, (coarse, half, fine, states, cc, fc, cc + fc + states, max(cc, fc)) + plan(n, max(cc, fc), T, M, flags, scratch_mb)


@dataclass
class WeakResult:
    sat_id: int
    doppler_hz: float
    code_phase: int
    carrier_phase: float
    z: float
    peak_ratio: float
    set: int
    coarse_doppler_hz: float
    z_margin: float           # (best z - runner-up z) / best z: the smaller of the two levels' margins


def _best(cells: Sequence[HybridCell]) -> Tuple[int, float]:
    zs = np.array([c.z for c in cells])
    ok = ~np.isnan(zs)
    if not ok.any():
        return 0, 1.0
    i = int(np.argmax(np.where(ok, zs, -np.inf)))        # lowest bin wins a tie, NaN never wins
    rest = np.where(ok, zs, -np.inf)
    rest[i] = -np.inf
    return i, float((zs[i] - rest.max()) / abs(zs[i])) if np.isfinite(rest.max()) else 1.0


def acquire_weak(iq: np.ndarray, fs: int, n: int, sat_ids: Sequence[int], T: int, M: int, flags: int, center: float = 0.0,
                 spread: float = 7000.0, fine_step: float = 10.0, replicas: Optional[Dict[int, np.ndarray]] = None) -> List[WeakResult]:
    sat_ids = list(sat_ids)
    spectra = replica_conj_spectra(n, sat_ids)
    bins = coarse_bins(center, spread, T)
    grid: List[List[HybridCell]] = [[] for _ in sat_ids]           # [satellite][bin]
    for f in bins:
        prof = block_profiles_shared(iq, fs, n, sat_ids, f, T, M, spectra)
        for k, sv in enumerate(sat_ids):
            grid[k].append(hybrid_cell(iq, fs, n, sv, f, T, M, flags, profiles=prof[k]))
    out = []
    for k, sv in enumerate(sat_ids):
        i, margin = _best(grid[k])
        coarse = bins[i]
        f_best, c_best = bins[i], grid[k][i]
        fb = fine_bins(coarse, fine_step, T)
        if fb:
            cells = [hybrid_cell(iq, fs, n, sv, f, T, M, flags, profiles=block_profiles_shared(iq, fs, n, [sv], f, T, M, spectra[k:k + 1])[0]) for f in fb]
            i, fine_margin = _best(cells)
            margin = min(margin, fine_margin)
            f_best, c_best = fb[i], cells[i]
        cp = c_best.rec.argmax
        out.append(WeakResult(sv, f_best, cp, float(np.angle(c_best.C0[cp])), c_best.z, c_best.peak_ratio, c_best.set, coarse, margin))
    return out


def render(scene, code_doppler: bool = True, block_ms: int = 50) -> np.ndarray:
    """`synth.render` with code Doppler: the code time of sample n is (n - cp) (1 + d / 1575.42e6) samples and the sample holds the
    chip at its CENTRE, chip floor((code time + 0.5) / up) mod 1023 (up = samples per chip), so the correlation peak sits at
    cp - round(n d / 1575.42e6) after n samples.  With d = 0 this is synth.render's roll(repeat(chips, up), cp) exactly.

    Why the centre: with an integer cp and a whole number of samples per chip the sample instants n lie exactly ON the chip edges,
    where an arbitrarily small stretch decides which chip a sample holds -- a negative Doppler would move the whole peak one sample
    late from the first millisecond on, a positive one would hold it in place until the drift is a full sample (the peak at
    cp - floor(drift)): an artefact of that degenerate lattice, not of code Doppler.  No front end samples on the chip edges; at
    the centres the chip of a sample is robust and the sampled peak follows the drift rounded to the nearest sample.
    complex64[n_ms * N]."""
    from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table

    n, fs = scene.samples_per_ms, scene.fs
    chips = generate_ca_code_table().astype(np.float64) * 2 - 1
    up = n // 1023
    out = np.empty(scene.n_ms * n, dtype=np.complex64)
    rng = np.random.default_rng(scene.seed)
    for b0 in range(0, scene.n_ms, block_ms):
        b1 = min(scene.n_ms, b0 + block_ms)
        idx = np.arange(b0 * n, b1 * n, dtype=np.float64)
        acc = np.zeros((b1 - b0) * n, dtype=complex)
        for s in scene.sats:
            stretch = 1.0 + (s.doppler_hz / 1575.42e6 if code_doppler else 0.0)
            chip = np.floor(((idx - s.code_phase) * stretch + 0.5) / up).astype(np.int64) % 1023
            sig = s.amplitude * chips[s.sat_id - 1][chip] * np.exp(1j * (2 * np.pi * s.doppler_hz * idx / fs + s.carrier_phase))
            if s.nav_bits is not None:
                ms = np.arange(b0, b1) + s.nav_bit_offset_ms
                bits = s.nav_bits[(ms // 20) % len(s.nav_bits)].astype(np.float64)
                sig = sig * np.repeat(bits, n)
            acc += sig
        noise = rng.standard_normal((b1 - b0) * n) + 1j * rng.standard_normal((b1 - b0) * n)
        acc += scene.noise_sigma * noise
        out[b0 * n:b1 * n] = acc.astype(np.complex64)
    return out
