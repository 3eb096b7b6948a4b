"""numpy float64 model of the weak-signal measurement (include/gypsum_hip.h, "weak-signal measurement"): the open-loop three-lag sums
and W_m of step 2 from tests/weak_track_model.py, steps 3-5 restated from the header, the refusals, the state a weak bank takes, and
a renderer that places satellites at FRACTIONAL code phases, with code Doppler, sampled at the sample centres.

`fold` walks the groups in the header's order in Python floats (one IEEE rounding per operation, math.sqrt correctly rounded), so on
the same float32 sums and W_m the library's host form gives the same dd and c0 bit for bit; the C/N0 goes through log10 and agrees to
about 1e-12.  The sums themselves are float64 here with numpy's exp and float32 on the device with its polynomial carrier.

`python tests/weak_measure_model.py` prints what tests/test_weak_measure_host.py gates and records: per scene (C/N0, Doppler, buffer)
over SEEDS, from a start drawn uniformly within half a sample of the truth and a Doppler 0.2 Hz off, the rms of the start error, the
rms and the largest final error of c0 in chips, and the mean and the largest error of the C/N0 estimate.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

import weak_track_model as wm

MIN_MS, MAX_MS, MAX_PASSES = 40, 2000, 4
MIN_SPACING, MAX_SPACING = 1 << 36, 1 << 39
ONE, CODE_MOD = wm.ONE, wm.CODE_MOD


@dataclass
class Params:
    spacing: int = 1 << 39
    passes: int = 2


@dataclass
class Fold:
    e_minus: float
    e_prompt: float
    e_plus: float
    wn: float
    dd: float
    cn0_dbhz: float
    c0: int
    n_groups: int
    status: int


@dataclass
class Measured:
    c0: int
    code_phase_samples: float
    delta_chips: float
    dd_last: float
    cn0_dbhz: float
    n_groups: int
    status: int
    folds: List[Fold] = field(default_factory=list)
    sums: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = field(default_factory=list)    # per pass: minus, prompt, plus complex128[n_ms]
    w: List[np.ndarray] = field(default_factory=list)


def refusal(p: Params, n_ms: int, first_ms: int) -> Optional[str]:
    """measure_refusal: why a request is refused, in the header's order (the candidates come after: cand_refusal)."""
    if not MIN_SPACING <= p.spacing <= MAX_SPACING:
        return "spacing must be 2^36 .. 2^39"
    if not 1 <= p.passes <= MAX_PASSES:
        return "passes must be 1..4"
    if not MIN_MS <= n_ms <= MAX_MS:
        return "n_ms must be 40..2000"
    if first_ms < 0:
        return "first_ms is negative"
    return None


def first_head(first_ms: int, edge: int) -> int:
    """The first group's head as an index into the buffer."""
    return (edge - first_ms) % 20


def n_groups(n_ms: int, first_ms: int, edge: int) -> int:
    left = n_ms - first_head(first_ms, edge)
    return left // 20 if left >= 20 else 0


def edge_refusal(edge: int, n_ms: int, first_ms: int) -> Optional[str]:
    if not 0 <= edge <= 19:
        return "an edge is outside 0..19"
    if n_groups(n_ms, first_ms, edge) < 1:
        return "no whole group of 20 milliseconds at an edge"
    return None


def cand_refusal(stream: int, sat_id: int, doppler_hz: float, carrier_phase: float, code_phase: int, edge: int, n: int, n_ms: int,
                 first_ms: int) -> Optional[str]:
    why = wm.init_refusal(stream, sat_id, doppler_hz, carrier_phase)
    if why:
        return why
    if not 0 <= code_phase < n:
        return "a code phase is outside [0, N)"
    return edge_refusal(edge, n_ms, first_ms)


def open_loop_sums(x: np.ndarray, chips_pm: np.ndarray, fs: int, n: int, f: float, u0: float, c0: int, n_ms: int, spacing: int):
    """Step 2 of one pass: (minus, prompt, plus complex128[n_ms], W float64[n_ms]) from the pass's c0."""
    r = wm.code_rate(f, n)
    out = np.zeros((3, n_ms), dtype=np.complex128)
    w = np.zeros(n_ms)
    for m in range(n_ms):
        x_ms = x[m * n:(m + 1) * n]
        out[:, m] = wm.ms_sums(x_ms, chips_pm, fs, u0, f, 0, c0, r, spacing)
        xr, xi = x_ms.real.astype(np.float64), x_ms.imag.astype(np.float64)
        w[m] = float(np.sum(xr * xr + xi * xi))
        u0, c0 = wm.advance(u0, c0, f, fs, n, r)
    return out[0], out[1], out[2], w


def cn0(e_prompt: float, wn: float) -> float:
    if not wn > 0.0 or not e_prompt > wn:
        return float("nan")
    snr = (e_prompt - wn) / wn
    return 10.0 * math.log10(snr / 0.020)


def fold(minus: np.ndarray, prompt: np.ndarray, plus: np.ndarray, w: np.ndarray, first_ms: int, edge: int, spacing: int, c0: int) -> Fold:
    """Steps 3-4 of one pass.  minus, prompt, plus: the per-millisecond sums (rounded to complex64 here, as the device stores them)."""
    n_ms = len(w)
    lags = [np.asarray(v).astype(np.complex64) for v in (minus, prompt, plus)]
    head, groups = first_head(first_ms, edge), n_groups(n_ms, first_ms, edge)
    tot = [0.0, 0.0, 0.0, 0.0]
    for g in range(groups):
        h = head + 20 * g
        for k, v in enumerate(lags):
            re = im = 0.0
            for j in range(h, h + 20):
                re += float(v[j].real)
                im += float(v[j].imag)
            a, b = re * re, im * im
            tot[k] += a + b
        ws = 0.0
        for j in range(h, h + 20):
            ws += float(w[j])
        tot[3] += ws
    em, ep, el, wn = tot

    def envelope(e: float) -> float:
        over = e - wn
        return math.sqrt(over if over > 0.0 else 0.0)

    a_minus, a_plus = envelope(em), envelope(el)
    total = a_plus + a_minus
    dd, status = 0.0, 1
    if total > 0.0:
        gain = 1.0 - float(spacing) / float(ONE)
        dd, status = gain * (a_plus - a_minus) / total, 0
    return Fold(em, ep, el, wn, dd, cn0(ep, wn), (c0 + wm.llround(dd * float(ONE))) % CODE_MOD, groups, status)


def code_phase_samples(c0: int, n: int) -> float:
    """The inverse of the start rule: 0.5 - K (c0 / 2^40), + N when negative, 0 where that rounds to N."""
    cp = 0.5 - float(n // 1023) * (float(c0) / float(ONE))
    if cp < 0.0:
        cp += float(n)
    return cp if cp < float(n) else 0.0


def measure(x: np.ndarray, chips_pm: np.ndarray, fs: int, n: int, doppler_hz: float, carrier_phase: float, code_phase: int, edge: int,
            first_ms: int, n_ms: int, p: Params = Params(), keep: bool = False) -> Measured:
    """Steps 1-5 for one candidate over the first n_ms milliseconds of x."""
    f, u0, c0 = float(doppler_hz), wm.init_u0(carrier_phase), wm.init_c0(code_phase, n)
    out = Measured(c0, 0.0, 0.0, 0.0, float("nan"), 0, 0)
    for _ in range(p.passes):
        mi, pr, pl, w = open_loop_sums(x, chips_pm, fs, n, f, u0, c0, n_ms, p.spacing)
        fo = fold(mi, pr, pl, w, first_ms, edge, p.spacing, c0)
        c0 = fo.c0
        out.delta_chips = out.delta_chips + fo.dd
        out.status |= fo.status
        out.folds.append(fo)
        if keep:
            out.sums.append((mi, pr, pl))
            out.w.append(w)
    last = out.folds[-1]
    out.c0, out.code_phase_samples, out.dd_last, out.cn0_dbhz, out.n_groups = c0, code_phase_samples(c0, n), last.dd, last.cn0_dbhz, last.n_groups
    return out


def state(doppler_hz: float, carrier_phase: float, c0: int, edge: int, fs: int, n: int, ms_ahead: int) -> dict:
    """gyp_weak_measured_state: f, f_int, u0, c0, phase, edge after ms_ahead open-loop milliseconds."""
    f, u0 = float(doppler_hz), wm.init_u0(carrier_phase)
    r = wm.code_rate(f, n)
    for _ in range(ms_ahead):
        u0, c0 = wm.advance(u0, c0, f, fs, n, r)
    return dict(f=f, f_int=f, u0=u0, c0=c0, phase=wm.WAIT, edge=edge)


# ---------------------------------------------------------------------------------------------- the scene
@dataclass
class Sat:
    sat_id: int
    doppler_hz: float
    code_phase: float          # the sample, with its fraction, at which chip 0 begins
    carrier_phase: float
    amplitude: float
    bits: np.ndarray           # +-1 per 20 ms
    bit_offset_ms: int         # millisecond i of the buffer starts a bit when (i + bit_offset_ms) % 20 == 0


def render(sats: List[Sat], fs: int, n: int, n_ms: int, sigma: float, seed: int, block_ms: int = 50) -> np.ndarray:
    """hybrid_model.render with a fractional code phase: the code time of sample k is (k - code_phase) (1 + d / 1575.42e6) samples and
    the sample holds the chip at its centre, chip floor((code time + 0.5) / up) mod 1023.  complex64[n_ms * N]."""
    from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table
    chips = generate_ca_code_table().astype(np.float64) * 2 - 1
    up = n // 1023
    out = np.empty(n_ms * n, dtype=np.complex64)
    rng = np.random.default_rng(seed)
    for b0 in range(0, n_ms, block_ms):
        b1 = min(n_ms, b0 + block_ms)
        idx = np.arange(b0 * n, b1 * n, dtype=np.float64)
        acc = np.zeros((b1 - b0) * n, dtype=complex)
        for s in sats:
            stretch = 1.0 + s.doppler_hz / wm.L1_HZ
            chip = np.floor(((idx - s.code_phase) * stretch + 0.5) / up).astype(np.int64) % 1023
            ms = np.arange(b0, b1) + s.bit_offset_ms
            bits = s.bits[(ms // 20) % len(s.bits)].astype(np.float64)
            acc += s.amplitude * chips[s.sat_id - 1][chip] * np.exp(1j * (2 * np.pi * s.doppler_hz * idx / fs + s.carrier_phase)) * np.repeat(bits, n)
        acc += sigma * (rng.standard_normal((b1 - b0) * n) + 1j * rng.standard_normal((b1 - b0) * n))
        out[b0 * n:b1 * n] = acc.astype(np.complex64)
    return out


def true_c0(s: Sat, n: int) -> float:
    """The code phase in chips at the centre of the buffer's first sample, as render places it."""
    return ((0.5 - s.code_phase * (1.0 + s.doppler_hz / wm.L1_HZ)) / (n // 1023)) % 1023.0


def code_error(c0: int, s: Sat, n: int) -> float:
    """c0 against the truth, in chips, wrapped to +-511.5."""
    return (c0 / ONE - true_c0(s, n) + 511.5) % 1023.0 - 511.5


FS, N, SIGMA = 2_046_000, 2046, 0.05
SEEDS = tuple(range(1, 9))
DOPPLER_OFF_HZ = 0.2
#         name                          sat  C/N0   Doppler  n_ms  gated
SCENES = (("30 dB-Hz 4487 Hz 220 ms", 7, 30.0, 4487.0, 220, True),
          ("33 dB-Hz -3950 Hz 220 ms", 15, 33.0, -3950.0, 220, True),
          ("45 dB-Hz 4100 Hz 220 ms", 3, 45.0, 4100.0, 220, True),
          ("30 dB-Hz 1233 Hz 1000 ms", 26, 30.0, 1233.0, 1000, True),
          ("30 dB-Hz 1233 Hz 220 ms", 26, 30.0, 1233.0, 220, False),
          ("45 dB-Hz -2871 Hz 220 ms", 3, 45.0, -2871.0, 220, False))


def amplitude(cn0_dbhz: float, n: int = N, sigma: float = SIGMA) -> float:
    """C/N0 = A^2 / (2 sigma^2) x fs, fs = 1000 N: as tests/weak_track_scene.py."""
    return sigma * math.sqrt(2.0 * 10.0 ** (cn0_dbhz / 10.0) / (1000.0 * n))


def chips_pm(sat_id: int) -> np.ndarray:
    from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table
    return generate_ca_code_table()[sat_id - 1].astype(np.float64) * 2 - 1


def drift_samples(doppler_hz: float, n_ms: int, n: int = N) -> float:
    """How far the code drifts against the sample grid over the buffer, in samples."""
    return abs(doppler_hz) / wm.L1_HZ * n_ms * n


def one_case(sat_id: int, cn0_dbhz: float, doppler_hz: float, n_ms: int, seed: int, p: Params = Params()):
    """(the satellite, the buffer, the candidate: doppler, carrier phase, integer code phase, edge, first_ms).  The start is the sample
    grid's: the true fractional code phase is the integer one plus a uniform draw within half a sample."""
    rng = np.random.default_rng([seed, sat_id, n_ms, 0x3EA5])
    cp_int = int(rng.integers(0, N))
    off = int(rng.integers(0, 20))
    s = Sat(sat_id, doppler_hz, cp_int + float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-np.pi, np.pi)), amplitude(cn0_dbhz),
            (rng.integers(0, 2, n_ms // 20 + 2) * 2 - 1).astype(np.int8), off)
    x = render([s], FS, N, n_ms, SIGMA, seed * 1000 + sat_id)
    first_ms = int(rng.integers(0, 1000))
    edge = (first_ms - off) % 20
    return s, x, dict(doppler_hz=doppler_hz + DOPPLER_OFF_HZ, carrier_phase=s.carrier_phase, code_phase=cp_int, edge=edge, first_ms=first_ms)


def scene_figures(sat_id: int, cn0_dbhz: float, doppler_hz: float, n_ms: int, seeds=SEEDS, p: Params = Params()) -> dict:
    start, final, cn0_err = [], [], []
    for seed in seeds:
        s, x, c = one_case(sat_id, cn0_dbhz, doppler_hz, n_ms, seed, p)
        m = measure(x, chips_pm(sat_id), FS, N, c["doppler_hz"], c["carrier_phase"], c["code_phase"], c["edge"], c["first_ms"], n_ms, p)
        start.append(code_error(wm.init_c0(c["code_phase"], N), s, N))
        final.append(code_error(m.c0, s, N))
        cn0_err.append(m.cn0_dbhz - cn0_dbhz)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    return dict(start_rms=rms(start), final_rms=rms(final), final_max=float(np.max(np.abs(final))), cn0_mean=float(np.mean(cn0_err)) + cn0_dbhz,
                cn0_err_max=float(np.max(np.abs(cn0_err))), drift=drift_samples(doppler_hz, n_ms))


# ---------------------------------------------------------------------------------------------- the route's scene
# Two 30 dB-Hz satellites whose code drifts more than a sample over the search's 220 ms, at fractional code phases; 1000 ms.
ROUTE_MS, ROUTE_SEARCH_MS, ROUTE_SEED = 1000, 220, 2
ROUTE_SPEC = ((7, 4487.0, 812.37, 5), (19, -4462.0, 1650.71, 10))      # satellite, Doppler, code phase in samples, bit offset
GOLDEN = Path(__file__).resolve().parent / "golden" / "weak_measure_route.npz"


def route_sats(seed: int = ROUTE_SEED) -> List[Sat]:
    rng = np.random.default_rng([seed, 0x5EA7])
    return [Sat(sv, d, cp, float(rng.uniform(-np.pi, np.pi)), amplitude(30.0), (rng.integers(0, 2, ROUTE_MS // 20 + 2) * 2 - 1).astype(np.int8), off)
            for sv, d, cp, off in ROUTE_SPEC]


def route_iq(seed: int = ROUTE_SEED) -> np.ndarray:
    return render(route_sats(seed), FS, N, ROUTE_MS, SIGMA, seed)


def route_bit(s: Sat, first_ms: int) -> int:
    return int(s.bits[((first_ms + s.bit_offset_ms) // 20) % len(s.bits)])


def route_model(seed: int = ROUTE_SEED, search=None) -> List[dict]:
    """The model's route for each satellite: the search's result (hybrid_model.acquire_weak; ten seconds -- or `search`, rows of
    (doppler_hz, carrier_phase, code_phase)), refined and measured on the first 220 ms, then one channel put in WAIT from the measured
    state and one started in SYNC from the refined result, both over the whole scene."""
    import hybrid_model as hm
    import weak_refine_model as rm
    sats, x = route_sats(seed), route_iq(seed)
    head = x[:ROUTE_SEARCH_MS * N]
    if search is None:
        res = hm.acquire_weak(head, FS, N, [s.sat_id for s in sats], 10, ROUTE_SEARCH_MS // 10, hm.ALTERNATE | hm.CODE_DOPPLER, 0.0, 7000.0, 10.0)
        search = [(r.doppler_hz, r.carrier_phase, r.code_phase) for r in res]
    out = []
    for s, (f0, ph0, cp) in zip(sats, search):
        chips = chips_pm(s.sat_id)
        f, ph, est = rm.refine(head, chips, FS, N, f0, ph0, cp, ROUTE_SEARCH_MS)
        m = measure(head, chips, FS, N, f, ph, cp, est.edge, 0, ROUTE_SEARCH_MS)
        a = wm.Channel.from_init(FS, N, chips, wm.Params(), f, ph, cp, 0)
        a.set_state(f, f, wm.init_u0(ph), m.c0, est.edge)
        b = wm.Channel.from_init(FS, N, chips, wm.Params(), f, ph, cp, 0)
        _, (pa, pb) = wm.run(x, [a, b], ROUTE_MS)
        out.append(dict(sat=s, search=(f0, ph0, cp), doppler_hz=f, carrier_phase=ph, edge=est.edge, measured=m, from_measured=pa, from_sync=pb,
                        code_error=code_error(m.c0, s, N), start_error=code_error(wm.init_c0(cp, N), s, N)))
    return out


def route_figures(r: dict) -> dict:
    s, pa, pb = r["sat"], r["from_measured"], r["from_sync"]
    wrong = sum(1 for p in pa if p.bit != route_bit(s, p.first_ms))
    return dict(wrong=min(wrong, len(pa) - wrong), n_bits=len(pa), first_a=pa[0].first_ms, first_b=pb[0].first_ms,
                dd_a=float(np.mean([abs(p.dd) for p in pa[:5]])), dd_b=float(np.mean([abs(p.dd) for p in pb[:5]])))


def route_golden() -> dict:
    with np.load(GOLDEN) as g:
        assert int(g["seed"]) == ROUTE_SEED
        return {k: g[k] for k in g.files}


def write_route_golden() -> None:
    rows = route_model()
    fig = [route_figures(r) for r in rows]
    np.savez_compressed(GOLDEN, seed=np.int64(ROUTE_SEED), search=np.array([r["search"] for r in rows]), doppler_hz=np.array([r["doppler_hz"] for r in rows]),
                        carrier_phase=np.array([r["carrier_phase"] for r in rows]), edge=np.array([r["edge"] for r in rows], dtype=np.int32),
                        c0=np.array([r["measured"].c0 for r in rows], dtype=np.int64), cn0_dbhz=np.array([r["measured"].cn0_dbhz for r in rows]),
                        dd_last=np.array([r["measured"].dd_last for r in rows]), code_error=np.array([r["code_error"] for r in rows]),
                        start_error=np.array([r["start_error"] for r in rows]), wrong=np.array([f["wrong"] for f in fig], dtype=np.int32),
                        n_bits=np.array([f["n_bits"] for f in fig], dtype=np.int32), first_measured=np.array([f["first_a"] for f in fig], dtype=np.int64),
                        first_sync=np.array([f["first_b"] for f in fig], dtype=np.int64), dd_measured=np.array([f["dd_a"] for f in fig]),
                        dd_sync=np.array([f["dd_b"] for f in fig]),
                        bits_measured=np.array([[p.bit for p in r["from_measured"]][:40] for r in rows], dtype=np.int8))


def report_route(seed: int) -> None:
    for r in route_model(seed):
        g, m = route_figures(r), r["measured"]
        print(f"seed {seed} sat {r['sat'].sat_id}: search {r['search']} refined {r['doppler_hz']:.3f} Hz edge {r['edge']} (true {(-r['sat'].bit_offset_ms) % 20}); "
              f"code error {r['start_error']:+.3f} -> {r['code_error']:+.3f} chip, dd_last {m.dd_last:+.4f}, C/N0 {m.cn0_dbhz:.2f}; from the measured state "
              f"{g['wrong']} wrong bits of {g['n_bits']}, first bit at {g['first_a']} ms (from SYNC {g['first_b']}), mean |dd| of five {g['dd_a']:.4f} (from SYNC {g['dd_b']:.4f})")


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] == ["--route"]:
        for a in sys.argv[2:] or [str(ROUTE_SEED)]:
            report_route(int(a))
        sys.exit(0)
    if sys.argv[1:] == ["--write-golden"]:
        write_route_golden()
        print(f"wrote {GOLDEN}")
        sys.exit(0)
    for name, sv, c, d, n_ms, gated in SCENES:
        g = scene_figures(sv, c, d, n_ms)
        print(f"{name} ({'gated' if gated else 'lattice-limited'}, drift {g['drift']:.2f} samples): start rms {g['start_rms']:.3f} final rms {g['final_rms']:.3f} "
              f"max {g['final_max']:.3f} chip; C/N0 mean {g['cn0_mean']:.2f}, largest error {g['cn0_err_max']:.2f} dB")
