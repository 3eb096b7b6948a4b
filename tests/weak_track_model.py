"""numpy float64 model of the weak bank (include/gypsum_hip.h, "weak-signal tracking"): the three-lag correlators, the bit
synchronisation and the 20-ms loops, restated from the header.

The integers are exact: code phases and rates are Python / int64 integers in units of 2^-40 chip, `code_rate`, `init_c0` and the chip
index of every sample are the header's expressions evaluated in the same order (numpy's float64 * / + are single IEEE roundings,
never contracted).  `bit_sync` is a bit-for-bit model of gyp_weak_bit_sync given the same float32 prompts.  The sums themselves are
float64 here with numpy's exp and float32 on the device with its polynomial carrier: they agree to the project's 1e-4 bar, not bitwise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

ONE = 1 << 40                      # one chip
CODE_MOD = 1023 * ONE
L1_HZ = 1575.42e6
SYNC, WAIT, TRACK = 0, 1, 2        # gyp_weak_state::phase
MU_WINDOW = 25


@dataclass
class Params:
    period_ms: int = 20
    spacing: int = ONE // 2
    sync_ms: int = 400
    pll_bw_hz: float = 8.0
    dll_bw_hz: float = 1.0
    lose_mu: float = 2.5


def llround(x: float) -> int:
    """C's llround: half away from zero (|x| - floor|x| is exact)."""
    whole = math.floor(abs(x))
    return int(whole + (1 if abs(x) - whole >= 0.5 else 0)) * (1 if x >= 0 else -1)


def frac(x: float) -> float:
    return float(np.float64(x) - np.floor(np.float64(x)))


def code_rate(f: float, n: int) -> int:
    return llround(float(np.float64(1023.0) / np.float64(n) * (np.float64(1.0) + np.float64(f) / np.float64(L1_HZ)) * np.float64(ONE)))


def init_c0(code_phase: int, n: int) -> int:
    k = n // 1023
    return llround(float((np.float64(0.5) - np.float64(code_phase)) / np.float64(k) * np.float64(ONE))) % CODE_MOD


def init_u0(carrier_phase: float) -> float:
    """frac(carrier_phase / 2 pi), and 0 where that rounds to 1 (a carrier phase a hair below zero): u0 stays in [0, 1)."""
    u = frac(float(np.float64(carrier_phase) / np.float64(2.0 * math.pi)))
    return u if u < 1.0 else 0.0


def chip_index(c_base: int, offset: int, k: np.ndarray, r: int) -> np.ndarray:
    """((c0 + o + k r) >> 40) mod 1023 for the int64 sample indices k: arithmetic shift, non-negative remainder."""
    return ((np.int64(c_base + offset) + k.astype(np.int64) * np.int64(r)) >> np.int64(40)) % np.int64(1023)


def ms_sums(x_ms: np.ndarray, chips_pm: np.ndarray, fs: int, u_base: float, f: float, k_first: int, c_base: int, r: int,
            spacing: int) -> Tuple[complex, complex, complex]:
    """minus, prompt, plus of one millisecond whose first sample is sample k_first of its period (float64)."""
    n = len(x_ms)
    k = np.arange(k_first, k_first + n, dtype=np.int64)
    du = np.float64(f) / np.float64(fs)
    u = np.float64(u_base) + du * k.astype(np.float64)
    w = np.asarray(x_ms).astype(np.complex128) * np.exp(-2j * np.pi * (u - np.rint(u)))
    return tuple(complex(np.sum(w * chips_pm[chip_index(c_base, o, k, r)])) for o in (-spacing, 0, spacing))


def bit_sync(prompts: np.ndarray, first_ms: int) -> Tuple[np.ndarray, int]:
    """gyp_weak_bit_sync: en[20] and the offset.  prompts: complex64[n_ms], the prompt of millisecond first_ms + i at i."""
    p = np.asarray(prompts, dtype=np.complex64)
    n_ms = len(p)
    en = np.zeros(20)
    for o in range(20):
        h = first_ms + (o - first_ms) % 20
        acc, groups = np.float64(0.0), 0
        while h + 20 <= first_ms + n_ms:
            re, im = np.float64(0.0), np.float64(0.0)
            for j in range(h - first_ms, h - first_ms + 20):
                re = re + np.float64(p[j].real)
                im = im + np.float64(p[j].imag)
            acc = acc + (re * re + im * im)
            groups += 1
            h += 20
        en[o] = acc / np.float64(groups) if groups else 0.0
    return en, int(np.argmax(en))               # np.argmax: the lowest index on a tie


def params_refusal(period_ms: int, sync_ms: int, spacing: int, pll_bw_hz: float, dll_bw_hz: float, lose_mu: float) -> Optional[str]:
    """weak_params_refusal: why a parameter set is refused, in the header's order."""
    if period_ms != 20:
        return "period_ms must be 20"
    if not 40 <= sync_ms <= 2000:
        return "sync_ms must be 40..2000"
    if not 1 <= spacing <= ONE:
        return "spacing must be 1 .. 2^40"
    if not 0.0 < pll_bw_hz <= 50.0:
        return "pll_bw_hz must be in (0, 50]"
    if not 0.0 < dll_bw_hz <= 10.0:
        return "dll_bw_hz must be in (0, 10]"
    if not 0.0 <= lose_mu <= 20.0:
        return "lose_mu must be in [0, 20]"
    return None


def init_refusal(stream: int, sat_id: int, doppler_hz: float, carrier_phase: float) -> Optional[str]:
    """weak_init_refusal."""
    if stream < 0:
        return "a stream index is negative"
    if not 1 <= sat_id <= 32:
        return "satellite id out of range"
    if not math.isfinite(doppler_hz):
        return "a Doppler is not finite"
    if not math.isfinite(carrier_phase):
        return "a carrier phase is not finite"
    return None


def advance(u0: float, c0: int, f: float, fs: float, samples: int, r: int) -> Tuple[float, int]:
    """weak_advance: u0 and c0 after `samples` samples at (f, r)."""
    du = np.float64(f) / np.float64(fs)
    return frac(float(np.float64(u0) + du * np.float64(samples))), (c0 + samples * r) % CODE_MOD


# weak_plan.hpp's WeakChan, as the host and the device hold it
CHAN = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("status", "<i4"), ("phase", "<i4"), ("edge", "<i4"), ("pos", "<i4"), ("n_periods", "<i4"),
                 ("sync_count", "<i4"), ("sync_start", "<i8"), ("period_first", "<i8"), ("f", "<f8"), ("f_int", "<f8"), ("u0", "<f8"), ("c0", "<i8"),
                 ("s_i", "<f8"), ("s_q", "<f8"), ("m_re", "<f8"), ("m_im", "<f8"), ("p_re", "<f8"), ("p_im", "<f8"), ("wbp", "<f8"),
                 ("mu", "<f8", (MU_WINDOW,)), ("mu_mean", "<f8")], align=True)
PERIOD_FIELDS = ("first_ms", "f", "u0", "c0", "i", "q", "mu", "dphi", "dd", "bit", "status", "mu_mean")


def fresh_chan(stream: int, sat_id: int, doppler_hz: float, carrier_phase: float, code_phase: int, n: int, cursor: int) -> np.ndarray:
    """weak_fresh_chan: one CHAN record in SYNC from millisecond `cursor`."""
    s = np.zeros(1, dtype=CHAN)[0]
    s["stream"], s["sat_id"], s["phase"], s["edge"], s["sync_start"] = stream, sat_id, SYNC, -1, cursor
    s["f"] = s["f_int"] = doppler_hz
    s["u0"], s["c0"] = init_u0(carrier_phase), init_c0(code_phase, n)
    return s


def fold_ms(s: np.ndarray, minus: complex, prompt: complex, plus: complex) -> None:
    """weak_fold_ms: one millisecond's float32 sums into the period's float64 sums of the CHAN record s."""
    pr, pi = np.float64(np.float32(prompt.real)), np.float64(np.float32(prompt.imag))
    s["s_i"] += pr
    s["s_q"] += pi
    s["m_re"] += np.float64(np.float32(minus.real))
    s["m_im"] += np.float64(np.float32(minus.imag))
    s["p_re"] += np.float64(np.float32(plus.real))
    s["p_im"] += np.float64(np.float32(plus.imag))
    s["wbp"] += pr * pr + pi * pi


def close_period(s: np.ndarray, p: Params, fs: float, n: int) -> dict:
    """weak_close_period on the CHAN record s (changed in place): the period record, as {PERIOD_FIELDS}.  Python floats and math.sqrt /
    math.atan: one IEEE rounding per operation, in the header's order."""
    T = p.period_ms / 1000.0
    two_pi = 2.0 * math.pi
    i, q = float(s["s_i"]), float(s["s_q"])
    m_re, m_im, p_re, p_im, wbp = (float(s[k]) for k in ("m_re", "m_im", "p_re", "p_im", "wbp"))
    e_minus, e_plus = math.sqrt(m_re * m_re + m_im * m_im), math.sqrt(p_re * p_re + p_im * p_im)
    nbp = i * i + q * q
    mu = nbp / wbp if wbp > 0.0 else 0.0
    dphi = math.atan(q / i) if i != 0.0 else 0.0
    e_sum = e_plus + e_minus
    dd = 0.5 * (e_plus - e_minus) / e_sum if e_sum != 0.0 else 0.0
    f = float(s["f"])
    rec = dict(first_ms=int(s["period_first"]), f=f, u0=float(s["u0"]), c0=int(s["c0"]), i=i, q=q, mu=mu, dphi=dphi, dd=dd, bit=1 if i >= 0.0 else -1, status=0)
    u0, c0 = advance(float(s["u0"]), int(s["c0"]), f, fs, p.period_ms * n, code_rate(f, n))
    wn = p.pll_bw_hz / 0.53
    kp, ki = 1.414 * wn, wn * wn
    s["f_int"] = float(s["f_int"]) + ki * dphi * T / two_pi
    s["f"] = float(s["f_int"]) + kp * dphi / two_pi
    s["u0"], s["c0"] = u0, (c0 + llround(4.0 * p.dll_bw_hz * dd * T * float(ONE))) % CODE_MOD
    s["mu"][int(s["n_periods"]) % MU_WINDOW] = mu
    s["n_periods"] += 1
    s["pos"] = 0
    for k in ("s_i", "s_q", "m_re", "m_im", "p_re", "p_im", "wbp", "mu_mean"):
        s[k] = 0.0
    if s["n_periods"] >= MU_WINDOW:
        total = 0.0
        for k in range(MU_WINDOW):                        # oldest first
            total += float(s["mu"][(int(s["n_periods"]) + k) % MU_WINDOW])
        s["mu_mean"] = total / MU_WINDOW
        if s["mu_mean"] < p.lose_mu:
            s["status"], rec["status"] = 2, 1
    rec["mu_mean"] = float(s["mu_mean"])
    return rec


@dataclass
class MsRec:
    minus: complex
    prompt: complex
    plus: complex
    phase: int
    pos: int
    status: int


@dataclass
class PeriodRec:
    first_ms: int
    f: float
    u0: float
    c0: int
    i: float
    q: float
    mu: float
    dphi: float
    dd: float
    bit: int
    status: int


@dataclass
class Channel:
    """One channel of the weak bank.  step() takes the millisecond at the cursor."""
    fs: int
    n: int
    chips_pm: np.ndarray               # the satellite's 1023 chips as +-1
    params: Params
    f: float
    u0: float
    c0: int
    cursor: int
    f_int: float = 0.0
    phase: int = SYNC
    edge: int = 0
    status: int = 0
    pos: int = 0
    sync_start: int = 0
    sync_prompts: List[complex] = field(default_factory=list)
    energies: Optional[np.ndarray] = None
    mus: List[float] = field(default_factory=list)
    lost_at_ms: Optional[int] = None
    period_first: int = 0
    acc: List[complex] = field(default_factory=list)   # this period's (minus, prompt, plus) per millisecond

    @classmethod
    def from_init(cls, fs: int, n: int, chips_pm: np.ndarray, params: Params, doppler_hz: float, carrier_phase: float, code_phase: int,
                  first_ms: int) -> "Channel":
        ch = cls(fs, n, chips_pm, params, float(doppler_hz), init_u0(carrier_phase), init_c0(code_phase, n), first_ms)
        ch.f_int = ch.f
        ch.sync_start = first_ms
        return ch

    def set_state(self, f: float, f_int: float, u0: float, c0: int, edge: int) -> None:
        self.f, self.f_int, self.u0, self.c0, self.edge = f, f_int, u0, c0, edge
        self.phase, self.status, self.pos, self.mus, self.acc = WAIT, 0, 0, [], []

    def _advance(self, samples: int, r: int) -> None:
        du = np.float64(self.f) / np.float64(self.fs)
        self.u0 = frac(float(np.float64(self.u0) + du * np.float64(samples)))
        self.c0 = (self.c0 + samples * r) % CODE_MOD

    def step(self, x_ms: np.ndarray) -> Tuple[MsRec, Optional[PeriodRec]]:
        m = self.cursor
        self.cursor += 1
        if self.status:
            return MsRec(0j, 0j, 0j, self.phase, 0, 2), None
        if self.phase == WAIT and m % 20 == self.edge:
            self.phase, self.pos = TRACK, 0
        p = self.params
        r = code_rate(self.f, self.n)
        if self.phase != TRACK:
            s = ms_sums(x_ms, self.chips_pm, self.fs, self.u0, self.f, 0, self.c0, r, p.spacing)
            rec = MsRec(*s, self.phase, 0, 0)
            self._advance(self.n, r)
            if self.phase == SYNC:
                self.sync_prompts.append(complex(np.complex64(s[1])))
                if len(self.sync_prompts) == p.sync_ms:
                    self.energies, self.edge = bit_sync(np.array(self.sync_prompts, dtype=np.complex64), self.sync_start)
                    self.phase = WAIT
            return rec, None
        if self.pos == 0:
            self.period_first, self.acc = m, []
        s = ms_sums(x_ms, self.chips_pm, self.fs, self.u0, self.f, self.pos * self.n, self.c0, r, p.spacing)
        rec = MsRec(*s, TRACK, self.pos, 0)
        self.acc.append(tuple(complex(np.complex64(v)) for v in s))     # the loops see the float32 sums, as on the device
        self.pos += 1
        if self.pos < p.period_ms:
            return rec, None
        return rec, self._close_period(r)

    def _close_period(self, r: int) -> PeriodRec:
        p = self.params
        T = p.period_ms / 1000.0
        sm = sp = sl = 0j
        wbp = np.float64(0.0)
        for mi, pr, pl in self.acc:                       # in order
            sm, sp, sl = sm + mi, sp + pr, sl + pl
            wbp = wbp + (np.float64(pr.real) * np.float64(pr.real) + np.float64(pr.imag) * np.float64(pr.imag))
        i, q = sp.real, sp.imag
        e_minus, e_plus = math.sqrt(sm.real * sm.real + sm.imag * sm.imag), math.sqrt(sl.real * sl.real + sl.imag * sl.imag)
        bit = 1 if i >= 0 else -1
        nbp = i * i + q * q
        mu = float(nbp / wbp) if wbp > 0 else 0.0
        dphi = math.atan(q / i) if i != 0 else 0.0
        dd = 0.5 * (e_plus - e_minus) / (e_plus + e_minus) if e_plus + e_minus != 0 else 0.0
        out = PeriodRec(self.period_first, self.f, self.u0, self.c0, i, q, mu, dphi, dd, bit, 0)
        self._advance(p.period_ms * self.n, r)
        wn = p.pll_bw_hz / 0.53
        kp, ki = 1.414 * wn, wn * wn
        self.f_int = self.f_int + ki * dphi * T / (2.0 * math.pi)
        self.f = self.f_int + kp * dphi / (2.0 * math.pi)
        self.c0 = (self.c0 + llround(4.0 * p.dll_bw_hz * dd * T * ONE)) % CODE_MOD
        self.mus.append(mu)
        self.pos = 0
        if len(self.mus) >= MU_WINDOW and sum(self.mus[-MU_WINDOW:]) / MU_WINDOW < p.lose_mu:
            self.status, out.status = 2, 1
            self.lost_at_ms = self.cursor
        return out

    def mu_mean(self) -> float:
        return sum(self.mus[-MU_WINDOW:]) / MU_WINDOW if len(self.mus) >= MU_WINDOW else float("nan")


def run(x: np.ndarray, channels: List[Channel], n_ms: int):
    """Every channel over the first n_ms milliseconds of x: (ms records [chan][ms], period records [chan][...])."""
    ms_out = [[] for _ in channels]
    per_out = [[] for _ in channels]
    for c, ch in enumerate(channels):
        for m in range(n_ms):
            rec, per = ch.step(x[m * ch.n:(m + 1) * ch.n])
            ms_out[c].append(rec)
            if per is not None:
                per_out[c].append(per)
    return ms_out, per_out
