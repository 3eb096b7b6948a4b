"""Weak-signal tracking, the parts that need no GPU: the golden file against the float64 model run afresh, the gates of the closed-loop
scene (tests/weak_track_scene.py) on the model and the oracle alone -- what tests/test_gpu_weak_track.py then holds the device to --,
gyp_weak_bit_sync and the defaults against the model, the record layouts against the header and the refusals that need no context."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weak_track_model as wm
import weak_track_scene as ws
from gypsum_amd import _lib, _records, engine
from oracle import gypsum_oracle as orc

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "gypsum_hip.h"


@pytest.fixture(scope="module")
def lib():
    from gypsum_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def model():
    return ws.model_run()


# ---------------------------------------------------------------------------------------------- the scene, on the model alone
def test_golden_is_the_model_run_afresh(model):
    fresh, g = ws.golden_arrays(), ws.golden()                             # the search for the three 30 dB-Hz satellites included
    assert sorted(fresh) == sorted(g)
    for k, v in fresh.items():
        assert np.asarray(v).dtype == g[k].dtype and np.array_equal(np.asarray(v), g[k]), k
    assert ws.GOLDEN.stat().st_size < 1 << 20


def test_bit_edge_is_found_for_every_present_satellite(model):
    chans, _, per = model
    tr = ws.truth()
    for c, sv in enumerate(ws.CHANNEL_SATS[:-1]):
        assert chans[c].edge == ws.true_edge(tr[sv]), sv
        assert per[c][0].first_ms == min(m for m in range(wm.Params().sync_ms, wm.Params().sync_ms + 20) if m % 20 == chans[c].edge)
        assert all(b.first_ms - a.first_ms == 20 for a, b in zip(per[c], per[c][1:]))


def test_no_wrong_bits_after_settling_at_30_dbhz_and_above(model):
    _, _, per = model
    tr = ws.truth()
    for c, sv in enumerate(ws.CHANNEL_SATS[:-1]):
        bad, n = ws.wrong_bits(tr[sv], per[c]), len(per[c]) - ws.SETTLE_PERIODS
        print(f"satellite {sv}: {bad} wrong bits of {n}")
        assert n >= 85
        if sv in ws.AT_LEAST_30:
            assert bad == 0, sv


def test_mu_of_present_satellites_and_loss_of_the_absent_channel(model):
    chans, ms, per = model
    for c, sv in enumerate(ws.CHANNEL_SATS[:-1]):
        print(f"satellite {sv}: smallest 25-period mu {ws.min_mu25(per[c]):.2f}")
        assert ws.min_mu25(per[c]) >= 4.0 and chans[c].status == 0 and chans[c].lost_at_ms is None, sv
    absent = len(ws.CHANNEL_SATS) - 1
    assert chans[absent].status == 2 and len(per[absent]) == 25 and per[absent][-1].status == 1
    assert chans[absent].lost_at_ms == per[absent][-1].first_ms + 20
    assert all(r.status == 2 for r in ms[absent][chans[absent].lost_at_ms:]) and all(r.status == 0 for r in ms[absent][:chans[absent].lost_at_ms])


def test_hand_off_from_the_recorded_search_results_gives_every_bit():
    """The model from what the model's weak-signal search returned for the 30 dB-Hz satellites (recorded in the golden file)."""
    g, tr = ws.golden(), ws.truth()
    assert tuple(g["search_sat"]) == ws.SEARCH_SATS
    for i, sv in enumerate(ws.SEARCH_SATS):
        assert abs(float(g["search_doppler_hz"][i]) - tr[sv].doppler_hz) <= 5.0 and int(g["search_code_phase"][i]) == tr[sv].code_phase
        ch, per = ws.track_from(ws.SEED, sv, float(g["search_doppler_hz"][i]), float(g["search_carrier_phase"][i]), int(g["search_code_phase"][i]))
        assert ch.edge == ws.true_edge(tr[sv]) and ws.wrong_bits(tr[sv], per) == 0 and ws.min_mu25(per) >= 4.0, sv


def test_false_lock_from_the_farther_search_bin_shows_in_phase_rms_alone(model):
    """The limit of the specified loop, held as a fact of the model: from the search's farther fine bin (7 or 8 Hz off) a 30 dB-Hz
    satellite ends in a false lock -- bits at chance, mu healthy, never lost -- and the rms of dphi over the last 25 periods is what
    tells it from lock.  The threshold 0.5 rad lies between the model's 0.13-0.30 (lock) and 0.74-1.06 (false lock) over nine seeds."""
    from gypsum_amd.weak_tracker import FALSE_LOCK_PHASE_RMS
    assert FALSE_LOCK_PHASE_RMS == 0.5
    _, _, per = model
    tr = ws.truth()
    for c, sv in enumerate(ws.CHANNEL_SATS[:-1]):
        print(f"satellite {sv}: phase rms {ws.phase_rms(per[c]):.3f}")
        assert ws.phase_rms(per[c]) < 0.35, sv
    for sv, f in ws.FAR_BIN_STARTS:
        ch, p = ws.track_from(ws.SEED, sv, f, 0.3, tr[sv].code_phase)
        n = len(p) - ws.SETTLE_PERIODS
        print(f"satellite {sv} from {f - tr[sv].doppler_hz:+.0f} Hz: wrong {ws.wrong_bits(tr[sv], p)} of {n}, mu25 {ws.min_mu25(p):.2f}, phase rms {ws.phase_rms(p):.3f}")
        assert ws.wrong_bits(tr[sv], p) > n // 3 and ch.status == 0 and ws.min_mu25(p) >= 4.0 and ws.phase_rms(p) > 0.7, sv


def test_reference_tracker_cannot_hold_a_30_dbhz_satellite():
    """oracle.Tracker, the reference's 1-ms loop, from the same start: its per-millisecond symbols agree with the data about as
    often as a coin (0.500 measured by the issue's author; the bar is 0.6), up to the sign."""
    sat = ws.truth()[7]
    init = ws.inits()[0]
    assert init["sat_id"] == 7
    prn = orc.prn_as_complex(orc.generate_ca_codes()[6], ws.N)
    trk = orc.Tracker(orc.TrackingState(init["doppler_hz"], init["carrier_phase"], init["code_phase"]), prn, ws.FS, ws.N)
    x = ws.iq()
    n_ms, agree = 1500, 0
    for m in range(n_ms):
        st, en = orc.chunk_times(m * ws.N, ws.N, ws.FS)
        rec = trk.process_samples(x[m * ws.N:(m + 1) * ws.N].astype(np.complex128), st, en)
        agree += int(rec.pseudosymbol == ws.true_bit(sat, m))
    share = max(agree, n_ms - agree) / n_ms
    print(f"reference tracker on satellite 7: agreement {share:.3f}")
    assert share < 0.6


# ---------------------------------------------------------------------------------------------- gyp_weak_bit_sync
def _prompts(rng, n_ms, first_ms, edge, amp=3.0):
    m = first_ms + np.arange(n_ms)
    bits = rng.integers(0, 2, n_ms // 20 + 3) * 2 - 1
    sig = amp * bits[(m - edge) // 20 - (first_ms - edge) // 20]
    return (sig + rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms)).astype(np.complex64)


def _check_sync(p, first_ms):
    en, off = engine.weak_bit_sync(p, first_ms)
    want_en, want_off = wm.bit_sync(p, first_ms)
    assert np.array_equal(en, want_en) and off == want_off          # bit for bit
    return en, off


def test_bit_sync_matches_the_model_bit_for_bit(lib):
    rng = np.random.default_rng(20261021)
    for n_ms, first_ms, edge in ((400, 0, 15), (400, 7, 3), (40, 0, 0), (2000, 123456789, 11), (41, 19, 19), (399, 21, 0), (60, 1, 1)):
        en, off = _check_sync(_prompts(rng, n_ms, first_ms, edge), first_ms)
        if n_ms >= 399:
            assert off == edge, (n_ms, first_ms, edge)


def test_bit_sync_tie_goes_to_the_lowest_offset(lib):
    p = np.zeros(60, dtype=np.complex64)
    p[:] = 1.0                                   # every group of every offset sums to 20: all twenty energies are 400
    en, off = _check_sync(p, 0)
    assert np.all(en == 400.0) and off == 0
    en, off = _check_sync(p, 13)                 # the same with a span that starts off a multiple of 20
    assert np.all(en == 400.0) and off == 0
    q = p.copy()
    q[5] = -1.0                                  # the groups that hold index 5 lose: offsets 6..19 tie at the top
    en, off = _check_sync(q, 0)
    assert off == 6 and en[6] == en[19] == 400.0 and en[5] < 400.0


def test_bit_sync_span_with_exactly_one_group(lib):
    rng = np.random.default_rng(5)
    p = (rng.standard_normal(20) + 1j * rng.standard_normal(20)).astype(np.complex64)
    for first_ms in (0, 20, 7, 999999):
        en, off = _check_sync(p, first_ms)       # only the offset of the span's first millisecond has a group; the others are 0
        assert off == first_ms % 20 and np.count_nonzero(en) == 1
        s = np.sum(p.astype(np.complex128))
        assert abs(en[off] - abs(s) ** 2) <= 1e-12 * abs(s) ** 2
    p39 = (rng.standard_normal(39) + 1j * rng.standard_normal(39)).astype(np.complex64)
    en, off = _check_sync(p39, 3)                # 39 ms: exactly one group for every offset
    assert np.count_nonzero(en) == 20


def test_bit_sync_first_ms_not_a_multiple_of_20(lib):
    rng = np.random.default_rng(6)
    base = _prompts(rng, 420, 0, 9)
    for cut in (1, 7, 19):
        en, off = _check_sync(base[cut:cut + 400], cut)
        assert off == 9


def test_bit_sync_refusals(lib):
    p = np.zeros(40, dtype=np.complex64)
    en = np.full(20, 7.0)
    off = np.full(1, 7, dtype=np.int32)
    for args in ((None, 40, 0), (_lib.ptr(p), 19, 0), (_lib.ptr(p), 40, -1)):
        assert lib.gyp_weak_bit_sync(args[0], args[1], args[2], _lib.ptr(en), _lib.ptr(off)) == _lib.GYP_E_BAD_ARG
    assert np.all(en == 7.0) and off[0] == 7
    assert lib.gyp_weak_bit_sync(_lib.ptr(p), 40, 0, None, None) == 0


# ---------------------------------------------------------------------------------------------- layouts, defaults, refusals
def test_weak_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_weak_params": _lib.WEAK_PARAMS, "gyp_weak_ms_rec": _lib.WEAK_MS_REC, "gyp_weak_period_rec": _lib.WEAK_PERIOD_REC,
               "gyp_weak_state": _lib.WEAK_STATE}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.strip().splitlines()}
    for name, dt in structs.items():
        assert got[(name, "size")] == dt.itemsize == _lib.RECORD_SIZES[name], name
        for field in dt.names:
            assert got[(name, field)] == dt.fields[field][1], (name, field)
    assert [dt.itemsize for dt in structs.values()] == [48, 32, 88, 64]
    assert _lib.GYP_VERSION == 209


def test_defaults_are_the_models(lib):
    d = engine.weak_params_default()[0]
    m = wm.Params()
    assert (int(d["period_ms"]), int(d["sync_ms"]), int(d["spacing"]), float(d["pll_bw_hz"]), float(d["dll_bw_hz"]), float(d["lose_mu"])) == \
        (m.period_ms, m.sync_ms, m.spacing, m.pll_bw_hz, m.dll_bw_hz, m.lose_mu) == (20, 400, 1 << 39, 8.0, 1.0, 2.5)
    assert _records.WeakParams().record().tobytes() == engine.weak_params_default().tobytes()
    assert _records.WeakParams.from_record(engine.weak_params_default()) == _records.WeakParams()


def test_model_integers():
    # the rate per sample: 2^39 at two samples per chip and no Doppler; carrier aiding moves it by f / 1575.42e6
    assert wm.code_rate(0.0, 2046) == 1 << 39 and wm.code_rate(0.0, 1023) == 1 << 40
    assert wm.code_rate(1575.42, 2046) - (1 << 39) == round((1 << 39) * 1e-6)
    # start-up: the centre of sample 0 is a quarter chip into chip 0 at code phase 0, K = 2; one sample earlier per unit of code phase
    assert wm.init_c0(0, 2046) == 1 << 38
    assert wm.init_c0(1, 2046) == wm.CODE_MOD - (1 << 38)
    assert wm.init_c0(2045, 2046) == (1 << 38) + (1 << 39)
    k = np.arange(5, dtype=np.int64)
    assert list(wm.chip_index(wm.init_c0(3, 2046), 0, k, 1 << 39)) == [1021, 1022, 1022, 0, 0]     # 3 samples before the wrap
    assert list(wm.chip_index(0, -1, k, 1 << 39)) == [1022, 0, 0, 1, 1]                              # a negative lag: floor, not truncation
    assert wm.llround(0.5) == 1 and wm.llround(-0.5) == -1 and wm.llround(2.4999) == 2 and wm.frac(-0.25) == 0.75


def test_entry_points_refuse_a_missing_bank_or_context(lib):
    p = _lib.ptr
    buf = np.zeros(16, dtype=np.float32)
    ms = np.zeros(1, dtype=_lib.WEAK_MS_REC)
    init = np.zeros(1, dtype=_lib.CHAN_INIT)
    st = np.zeros(1, dtype=_lib.WEAK_STATE)
    assert lib.gyp_weak_track_block_dev(None, p(buf), 2046, 0, 1, p(ms), None, None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_track_block(None, p(buf), 1, 0, 1, p(ms), None, None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_bank_create(None, p(init), 1, None, 0, None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_bank_size(None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_bank_set_channel(None, 0, p(init)) == lib.gyp_weak_bank_drop_channel(None, 0) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_bank_get_state(None, p(st), None) == lib.gyp_weak_bank_set_state(None, 0, p(st)) == _lib.GYP_E_BAD_ARG
    lib.gyp_weak_bank_destroy(None)
    assert not ms.tobytes().strip(b"\0") and not st.tobytes().strip(b"\0")
