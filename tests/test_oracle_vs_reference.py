"""Oracle and reference side by side.  The reference's outputs for these inputs are stored in tests/golden/oracle_vs_reference.npz
(tests/golden/make_golden.py `vsref` regenerates them by running the reference); the inputs are drawn here, from fixed seeds, and
their sha256 is stored beside the outputs."""
import hashlib

import numpy as np

import golden_util as gu


def _sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def correlator_cases():
    """(fs, n, sv, iq, peaks) of test_correlator_math, in the order the seeded generator draws them."""
    rng = np.random.default_rng(3)
    for fs in (2_046_000, 8_184_000):
        n = fs // 1000
        sv = int(rng.integers(1, 33))
        iq = (rng.standard_normal(3 * n + 17) + 1j * rng.standard_normal(3 * n + 17)).astype(np.complex64)
        peaks = rng.standard_normal(300) * 20 + 1j * rng.standard_normal(300)
        yield fs, n, sv, iq, peaks


def closed_loop_scene():
    from gypsum_amd import synth

    fs, n = 2_046_000, 2046
    scene = synth.random_scene(fs, 320, 4, 77, noise_sigma=0.02)
    return fs, n, scene.sats[0].sat_id, synth.render(scene)


def bit_fuzz_cases():
    """Random bit streams with flips, slips and junk: (pseudosymbols, start times, end times) per case."""
    rng = np.random.default_rng(77)
    for case in range(12):
        n_ms = int(rng.integers(200, 4000))
        bits = rng.integers(0, 2, n_ms // 20 + 3) * 2 - 1
        sym = np.repeat(bits, 20)[int(rng.integers(0, 20)):][:n_ms].astype(np.int8)
        sym = np.where(rng.random(n_ms) < rng.choice([0.0, 0.05, 0.2, 0.4]), -sym, sym)
        for _ in range(int(rng.integers(0, 4))):                     # slips: drop or repeat a few symbols
            at, k = int(rng.integers(100, n_ms - 30)), int(rng.integers(1, 19))
            sym = np.concatenate([sym[:at], sym[at + k:]]) if rng.random() < 0.5 else np.concatenate([sym[:at], sym[at - k:]])
        t0 = float(rng.choice([0.0, 37.5, 39.9]))
        start = np.round(t0 + np.arange(len(sym)) / 1000, 6)
        end = np.round(t0 + (np.arange(len(sym)) + 1) / 1000, 6)
        yield sym, start, end


def test_correlator_math():
    from oracle import gypsum_oracle as orc

    z = gu.load("oracle_vs_reference.npz")
    chips = orc.generate_ca_codes()
    for fs, n, sv, iq, peaks in correlator_cases():
        k = f"corr{fs}__"
        assert _sha(iq, peaks) == str(z[k + "inputs_sha256"]), "the seeded inputs changed (numpy RNG stream?)"
        assert sv == int(z[k + "sv"])
        prn = orc.prn_as_complex(chips[sv - 1], n)
        assert np.array_equal(prn, z[k + "prn"]) and prn.dtype == z[k + "prn"].dtype
        for kind, tag in ((orc.COHERENT, "coherent"), (orc.NON_COHERENT, "non_coherent")):
            a = orc.integrate_correlation(kind, iq, fs, n, 1234.5, prn)
            b = z[k + tag]
            assert a.dtype == b.dtype and np.array_equal(a, b), tag
        prof = np.abs(a)
        assert orc.peak_strength(prof) == float(z[k + "peak_strength"])
        assert orc.constellation_rotation(peaks) == float(z[k + "rotation"])
        assert orc.constellation_circularity(peaks) == float(z[k + "circularity"])


def test_acquisition_and_tracking_closed_loop():
    from oracle import gypsum_oracle as orc

    z = gu.load("oracle_vs_reference.npz")
    fs, n, sv, iq = closed_loop_scene()
    assert _sha(iq) == str(z["loop__iq_sha256"]), "the seeded scene changed (numpy RNG stream?)"
    assert sv == int(z["loop__sv"])
    chips = orc.generate_ca_codes()
    oa = orc.acquire_satellite(sv, iq[:10 * n], fs, n, orc.prn_as_complex(chips[sv - 1], n))
    assert (oa.doppler_shift, oa.prn_phase_shift, oa.correlation_strength, oa.carrier_wave_phase_shift) == tuple(z["loop__acquisition"])
    ot = orc.Tracker(orc.TrackingState(oa.doppler_shift, oa.carrier_wave_phase_shift, oa.prn_phase_shift),
                     orc.prn_as_complex(chips[sv - 1], n), fs, n)
    peak, doppler, carrier, code = z["loop__peak"], z["loop__doppler"], z["loop__carrier_phase"], z["loop__code_phase"]
    symbol, start, locked = z["loop__pseudosymbol"], z["loop__start_of_pseudosymbol"], z["loop__locked"]
    assert len(peak) == 320 - 9
    for j, ms in enumerate(range(9, 320)):
        t0, t1 = orc.chunk_times(ms * n, n, fs)
        rec = ot.process_samples(iq[ms * n:(ms + 1) * n], t0, t1)
        assert rec.peak == peak[j], ms
        assert rec.doppler_after == doppler[j], ms
        assert rec.carrier_phase_after == carrier[j], ms
        assert rec.code_phase_after == code[j], ms
        assert rec.pseudosymbol == symbol[j], ms
        assert rec.start_of_pseudosymbol == start[j], ms
        assert ot.s.is_locked() == bool(locked[j]), ms


def test_bit_integrator_fuzz():
    """Random bit streams with flips, slips and junk: reference, oracle and the native integrator agree event for event."""
    from gypsum_amd import _lib
    from gypsum_amd.navigation_bit_intergrator import NavigationBitIntegratorBank
    from oracle import gypsum_oracle as orc

    z = gu.load("oracle_vs_reference.npz")
    events, cursors = z["bits__events"], z["bits__cursors"]
    for case, (sym, start, end) in enumerate(bit_fuzz_cases()):
        assert _sha(sym, start, end) == str(z["bits__inputs_sha256"][case]), "the seeded inputs changed (numpy RNG stream?)"
        mine = events[events[:, 0] == case]
        want = [(float(a), float(b), int(c)) for a, b, c in mine[:, 1:]]
        at_want = cursors[cursors[:, 0] == case][:, 1]
        assert len(at_want) == len(sym)
        o = orc.BitIntegrator()
        got_o = []
        for v, st, en, at_ref in zip(sym, start, end, at_want):
            at, ev = o.process(float(st), float(st), float(en), int(v))
            assert at == at_ref
            got_o += ev
        assert got_o == want, case
        recs = np.zeros((1, len(sym)), dtype=_lib.TRACK_REC)
        recs["pseudosymbol"] = sym
        ev = NavigationBitIntegratorBank(1).push_block(recs, start, end)
        got_n = list(zip(ev["receiver_timestamp"].tolist(), ev["trailing_edge_receiver_timestamp"].tolist(), ev["bit_value"].tolist()))
        assert got_n == want, case
