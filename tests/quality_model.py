"""numpy float64 restatement of the signal-quality contract (include/gypsum_hip.h, "signal quality"): the per (channel, window) sums
of `track_quality_kernel` (gypsum_amd/csrc/kernels_quality.hpp) with its lane ownership, in-lane order and reduction tree, and the
host arithmetic of `quality_from_sums` (same file; gyp_quality_from_sums) in its stated order.

numpy's elementwise float64 +, *, / and sqrt are single IEEE roundings and never contracted, which is what the device code does
with contraction off; only log10 may differ from libm's by an ulp.
"""
from __future__ import annotations

import numpy as np

from gypsum_amd import _lib

LANES = 64
GROUP_MS = 20


def tree(acc: np.ndarray) -> np.generic:
    """The fixed tree: lane l takes lane l + 32, 16, 8, 4, 2, 1 (the __shfl_down loop of track_quality_kernel); lane 0's value."""
    acc = acc.copy()
    for off in (32, 16, 8, 4, 2, 1):
        acc[:off] = acc[:off] + acc[off:2 * off]
    return acc[0]


def window_sums(rec: np.ndarray, r0: int, r1: int, b: int) -> np.void:
    """One (channel, window): records [r0, r1) of the channel's row `rec`, bit offset b (-1..19) relative to the row's record 0."""
    out = np.zeros(1, dtype=_lib.QUALITY_SUMS)
    re, im = rec["peak_re"].astype(np.float64), rec["peak_im"].astype(np.float64)
    p2 = re * re + im * im                      # two exact products, one rounding
    p4 = p2 * p2
    used = rec["status"] != 2
    locked = rec["locked"] != 0
    lanes = np.arange(LANES)
    s2, s4 = np.zeros(LANES), np.zeros(LANES)
    n_used, n_locked = np.zeros(LANES, dtype=np.int64), np.zeros(LANES, dtype=np.int64)
    for first in range(r0, r1, LANES):          # lane l adds used records l, l + 64, ... of the window, in that order
        idx = first + lanes
        ok = idx < r1
        idx = np.where(ok, idx, r0)
        ok &= used[idx]
        s2[ok] = s2[ok] + p2[idx[ok]]
        s4[ok] = s4[ok] + p4[idx[ok]]
        n_used[ok] += 1
        n_locked[ok] += locked[idx[ok]]
    snp, spl = np.zeros(LANES), np.zeros(LANES)
    n_groups = np.zeros(LANES, dtype=np.int64)
    if b >= 0:
        g0 = 0 if r0 <= b else (r0 - b + GROUP_MS - 1) // GROUP_MS      # the window's first group: the first b + 20 g >= r0
        start0 = b + GROUP_MS * g0
        n_g = (r1 - start0) // GROUP_MS if start0 + GROUP_MS <= r1 else 0   # groups wholly inside [r0, r1)
        for j in range(n_g):                     # lane j % 64 owns the window's group j; a lane's groups come in increasing j
            s = start0 + GROUP_MS * j
            si = sq = wbp = np.float64(0.0)
            for k in range(s, s + GROUP_MS):     # in record order
                si = si + re[k]
                sq = sq + im[k]
                wbp = wbp + p2[k]
            ii, qq = si * si, sq * sq
            nbp, nbd = ii + qq, ii - qq
            if used[s:s + GROUP_MS].all() and wbp > 0.0 and nbp > 0.0:
                lane = j % LANES
                snp[lane] = snp[lane] + nbp / wbp
                spl[lane] = spl[lane] + nbd / nbp
                n_groups[lane] += 1
    o = out[0]
    o["n_used"], o["n_locked"], o["n_groups"] = n_used.sum(), n_locked.sum(), n_groups.sum()
    o["sum_p2"], o["sum_p4"], o["sum_np"], o["sum_pl"] = tree(s2), tree(s4), tree(snp), tree(spl)
    return out[0]


def track_quality(records: np.ndarray, window_ms: int, bit_offsets=None) -> np.ndarray:
    """(n_chan, ceil(n_ms / W)) QUALITY_SUMS of (n_chan, n_ms) TRACK_REC records: what gyp_track_quality(_dev) writes."""
    recs = np.asarray(records)
    n_chan, n_ms = recs.shape
    W = int(window_ms)
    n_win = -(-n_ms // W)
    out = np.zeros((n_chan, n_win), dtype=_lib.QUALITY_SUMS)
    for c in range(n_chan):
        b = -1 if bit_offsets is None else int(bit_offsets[c])
        for w in range(n_win):
            out[c, w] = window_sums(recs[c], w * W, min((w + 1) * W, n_ms), b)
    return out


def from_sums(sums) -> np.void:
    """gyp_quality_from_sums on the records of `sums` combined left to right (quality_from_sums, kernels_quality.hpp)."""
    s = np.asarray(sums, dtype=_lib.QUALITY_SUMS).reshape(-1)
    n_used, n_locked, n_groups = int(s["n_used"].astype(np.int64).sum()), int(s["n_locked"].astype(np.int64).sum()), int(s["n_groups"].astype(np.int64).sum())
    S2 = S4 = Snp = Spl = np.float64(0.0)
    for r in s:
        S2, S4, Snp, Spl = S2 + r["sum_p2"], S4 + r["sum_p4"], Snp + r["sum_np"], Spl + r["sum_pl"]
    out = np.zeros(1, dtype=_lib.QUALITY)
    q = out[0]
    q["cn0_m2m4_dbhz"] = q["cn0_nwpr_dbhz"] = q["phase_lock"] = q["locked_share"] = np.nan
    q["n_used"], q["n_groups"] = n_used, n_groups
    with np.errstate(all="ignore"):
        if n_used >= 2:
            n = np.float64(n_used)
            M2, M4 = S2 / n, S4 / n
            a = M2 * M2
            t = a + a
            d = t - M4
            if d > 0:
                Pd = np.sqrt(d)
                Pn = M2 - Pd
                if Pn > 0:
                    q["cn0_m2m4_dbhz"] = 10.0 * np.log10((Pd / Pn) * 1000.0)
        if n_groups >= 1:
            G = np.float64(n_groups)
            mu = Snp / G
            if mu > 1 and mu < 20:
                q["cn0_nwpr_dbhz"] = 10.0 * np.log10(((mu - 1.0) / (20.0 - mu)) * 1000.0)
            q["phase_lock"] = Spl / G
        if n_used >= 1:
            q["locked_share"] = np.float64(n_locked) / np.float64(n_used)
    return out[0]


def records_from_peaks(peaks: np.ndarray, status=None, locked=None) -> np.ndarray:
    """TRACK_REC rows whose prompt peaks are the complex64 `peaks` (any shape); the other fields 0 unless given."""
    p = np.asarray(peaks, dtype=np.complex64)
    rec = np.zeros(p.shape, dtype=_lib.TRACK_REC)
    rec["peak_re"], rec["peak_im"] = p.real, p.imag
    rec["pseudosymbol"] = np.where(p.real < 0, -1, 1)
    if status is not None:
        rec["status"] = status
    if locked is not None:
        rec["locked"] = locked
    return rec


def synthetic_peaks(a: float, v: float, n_ms: int, bit_offset: int, seed: int, phase: float = 0.1) -> np.ndarray:
    """complex64 prompt peaks A b e^{j phase} + noise of variance v per component, b = random 20-ms bits whose edges lie at
    bit_offset + 20 g."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n_ms // GROUP_MS + 2) * 2 - 1
    b = bits[(np.arange(n_ms) - bit_offset + GROUP_MS) // GROUP_MS]
    noise = np.sqrt(v) * (rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms))
    return (a * b * np.exp(1j * phase) + noise).astype(np.complex64)
