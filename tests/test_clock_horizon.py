"""Where closed-loop parity with the reference ends (oracle only, no device).

A Doppler update df moves the next millisecond's carrier phase by 2 pi df t (tracker.py:271-281 wipes the carrier off at absolute
receiver time), so the Costas loop's phase gain grows with t.  Past a few tens of seconds it amplifies every perturbation: the
float64 oracle and its own twin whose prompt peaks carry float32-sized perturbations (orc.Tracker.peak_noise = 3e-7, the suite's
float32 witness) then stop producing the same integers within 3 - 50 ms.  Near t = 0 they never do.  So "every integer equals the
oracle's" is a closed-loop bar only near t = 0; late in a recording the tests compare teacher-forced milliseconds, short loops inside
the horizon printed here, and what the device keeps bit for bit between its own paths (tests/test_gpu_clocks.py).
"""
from __future__ import annotations

import time

import pytest

import clock_model as cm

FS = 2_046_000
N_MS = cm.HORIZON_N_MS


@pytest.mark.parametrize("T,before_ms", [(0.0, None), (10.0, None), (40.0, 60), (3600.0, 30)])
def test_the_oracle_and_its_float32_twin_part_late_in_a_recording(T, before_ms):
    t_start = time.time()
    hs = cm.horizons(FS, T, N_MS)
    assert len(hs) == 4
    firsts = [None if h[0] is None else cm.HORIZON_FIRST_MS + h[0] for h in hs]
    print(f"[clock horizon T = {T:g} s] first millisecond with a different integer per channel {firsts} (of ms {cm.HORIZON_FIRST_MS} .. "
          f"{cm.HORIZON_FIRST_MS + N_MS - 1}), Doppler separation before it {[f'{h[1]:.1e}' for h in hs]} Hz, locked ms {[h[2] for h in hs]}; "
          f"horizon({T:g}) = {cm.horizon(FS, T, N_MS)} ms; {time.time() - t_start:.1f} s")
    if before_ms is None:
        assert firsts == [None] * 4, firsts
        assert max(h[1] for h in hs) < 1e-6, hs          # and the loops stay together: the twins' Doppler estimates within 1e-6 Hz
    else:
        assert all(f is not None and f < before_ms for f in firsts), firsts
        assert cm.horizon(FS, T, N_MS) == min(firsts) - cm.HORIZON_FIRST_MS


def test_clock_shapes():
    import numpy as np
    from oracle import gypsum_oracle as orc

    n, fs = 2046, 2_046_000
    s0, e0 = cm.clocks(n, fs, 5, "offset", 0.0, first_ms=9)
    assert [float(v) for v in s0] == [orc.chunk_times(ms * n, n, fs)[0] for ms in range(9, 14)] and np.array_equal(e0[:-1], s0[1:])
    s, e = cm.clocks(n, fs, 5, "offgrid", 40.0, first_ms=9)
    assert np.array_equal(s, s0 + 40.0 + cm.OFFGRID_S) and np.array_equal(e, e0 + 40.0 + cm.OFFGRID_S)
    s, _ = cm.clocks(n, fs, 5, "gapped", [(1, 2.5), (3, -1.0)], first_ms=9)
    assert np.allclose(s - s0, [0.0, 2.5, 2.5, 1.5, 1.5], rtol=0, atol=1e-12)
    s, e = cm.clocks(n, fs, 5, "per_stream", [0.0, 40.0, 3600.0], first_ms=9)
    assert s.shape == e.shape == (3, 5) and np.array_equal(s[0], s0) and np.array_equal(s[2], s0 + 3600.0)


@pytest.mark.parametrize("f", [4321.37, -4799.63, 0.37])
@pytest.mark.parametrize("t0", [40.009, 3600.001 + 1e-6 / 3, 604_800.123457])
def test_exact_start_has_the_exactly_reduced_phase(f, t0):
    from fractions import Fraction
    import math

    ts = cm.exact_start(f, t0)
    want = Fraction(f) * Fraction(t0)
    want -= math.floor(want)
    got = Fraction(f) * Fraction(ts)                      # the cycles the oracle's carrier then starts at, before ITS roundings
    d = abs(got - want)
    assert min(d, 1 - d) < 3e-16, float(d)               # two roundings of a number below 1
    assert abs(ts) <= 1.0 / abs(f)


def test_reference_noise_stays_inside_its_worst_case_up_to_one_gps_week():
    """The reference's own phase rounding (oracle against its exact-phase twin, three milliseconds of one channel): printed per start time
    (the table of DESIGN.md, "Clocks"), and never above its coherent worst case -- every sample's t = n / fs + t0 off by half an ulp of
    t0 and its argument 2 pi f t + phi rounded three times -- which at one GPS week is still 50 times below the 1e-4 bar."""
    import math
    import numpy as np
    from gypsum_amd import synth
    from oracle import gypsum_oracle as orc

    fs, n = 2_046_000, 2046
    scene = synth.random_scene(fs, 3, 3, 4102, max_doppler=4800.0, with_nav_bits=False)
    iq = synth.render(scene)
    sat = scene.sats[0]
    prn = orc.prn_as_complex(orc.generate_ca_codes()[sat.sat_id - 1], n)
    f, phi = sat.doppler_hz + 0.37, 0.8
    for T in (3600.0, 86_400.0, cm.GPS_WEEK_S, 1e9):
        worst = {"mag": 0.0, "angle": 0.0, "el": 0.0}
        for ms in range(3):
            t0 = float(cm.clocks(n, fs, 1, "offset", T, first_ms=ms)[0][0])
            got = cm.reference_noise(iq[ms * n:(ms + 1) * n], prn, fs, n, f, phi, sat.code_phase, t0)
            worst = {key: max(worst[key], got[key]) for key in worst}
        cap = 2 * math.pi * abs(f) * math.ulp(T) / 2 + 1.5 * math.ulp(2 * math.pi * abs(f) * T)
        print(f"[reference noise T = {T:g} s] relative |peak| difference {worst['mag']:.1e}, peak angle {worst['angle']:.1e} rad, early/late "
              f"{worst['el']:.1e} of the norm; coherent worst case {cap:.1e} rad")
        assert worst["angle"] <= cap and worst["mag"] <= cap and worst["el"] <= cap, (T, worst, cap)
        if T <= cm.GPS_WEEK_S:
            assert cap < 2e-6 * (T / cm.GPS_WEEK_S) + 1e-9
