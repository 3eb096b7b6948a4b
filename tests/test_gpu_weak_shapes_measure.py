"""gyp_weak_measure at its shape edges (the rows of tests/weak_shapes_scene.py; tests/test_weak_shapes_host.py holds them to their
group counts first): n_ms % 4 = 1, 2, 3 -- the ragged last workgroup of weak_measure_sums_kernel; 59 ms with a head of 19 and 60 ms
with a head of 1 -- two groups with no and with 19 spare milliseconds; 2000 ms with heads 0 and 19 -- 100 and 99 groups over the 128
threads of weak_measure_fold_kernel -- each under every setting of passes and spacing of tests/test_gpu_weak_measure.py.  At each:
pass 1's sums bit for bit against a weak bank in SYNC, W_m against numpy, every pass's fold against the host twin on the device's own
sums, the record from the folds, and on the two short rows the record against the float64 model.

Measured on an MI355X (printed by the model test): the record against the float64 model on the device's input differs by at most
5.2e-9 chip in c0 and 9.3e-8 dB in the C/N0 on the 59- and 60-ms rows -- the bars are 1e-4 chip and 1e-3 dB.
"""
from __future__ import annotations

import numpy as np
import pytest

import weak_measure_model as mm
import weak_shapes_scene as sc
import weak_track_model as wm
from gypsum_amd import _records, engine

pytestmark = pytest.mark.gpu

ROWS = list(range(len(sc.MEASURE_ROWS)))
_cases = {}


def case(engine_factory, k: int) -> dict:
    """Row k measured once per setting through the host form; shared by the tests below and left unchanged."""
    if k in _cases:
        return _cases[k]
    n_ms, start, head, _ = sc.MEASURE_ROWS[k]
    eng = engine_factory(sc.FS, sc.N)
    x = sc.head_of(sc.measure_iq(), n_ms, start)
    x.setflags(write=False)
    refined = sc.measure_refined(head)
    runs = {}
    for passes, spacing in sc.SETTINGS:
        runs[(passes, spacing)] = eng.measure_weak(x, 2, sc.FIRST_MS, refined, _records.WeakMeasureParams(spacing=spacing, passes=passes), want_sums=True)
        for a in runs[(passes, spacing)]:
            a.setflags(write=False)
    _cases[k] = dict(eng=eng, x=x, refined=refined, runs=runs)
    return _cases[k]


@pytest.mark.parametrize("k", ROWS, ids=sc.MEASURE_IDS)
def test_pass_1_sums_are_a_weak_banks_and_w_is_numpys(engine_factory, k):
    n_ms = sc.MEASURE_ROWS[k][0]
    c = case(engine_factory, k)
    x, refined = c["x"], c["refined"]
    power = []
    for s in (0, 1):
        xs = x[s].reshape(n_ms, sc.N).astype(np.complex128)
        power.append(np.sum(xs.real * xs.real + xs.imag * xs.imag, axis=1))
    for (passes, spacing), (rec, sums, w, folds) in c["runs"].items():
        assert sums.shape == w.shape == (4, passes, n_ms) and folds.shape == (4, passes)
        bank = c["eng"].create_weak_bank(sc.inits_of(refined), _records.WeakParams(sync_ms=n_ms, spacing=spacing), sc.FIRST_MS)
        try:
            ms, _ = bank.track_block(x, 2, sc.FIRST_MS, n_ms, want_periods=False)
        finally:
            bank.close()
        assert np.all(ms["phase"] == wm.SYNC) and np.all(ms["status"] == 0)
        assert sums[:, 0, :].tobytes() == ms.tobytes(), (passes, spacing)
        assert all(np.count_nonzero(sums[name]) == 4 * passes * n_ms for name in sc.SIX)          # every millisecond of every pass was written
        for i, r in enumerate(refined):
            want = power[int(r["stream"])]
            for p in range(passes):
                assert np.all(np.abs(w[i, p] - want) <= 1e-12 * want), (i, p)
                assert w[i, p].tobytes() == w[i, 0].tobytes()                                      # (and the same bits in every pass)


@pytest.mark.parametrize("k", ROWS, ids=sc.MEASURE_IDS)
def test_every_pass_is_the_twins_fold_and_the_record_follows(engine_factory, k):
    n_ms, _, head, groups = sc.MEASURE_ROWS[k]
    c = case(engine_factory, k)
    for (passes, spacing), (rec, sums, w, folds) in c["runs"].items():
        for i, r in enumerate(c["refined"]):
            c0 = wm.init_c0(int(r["code_phase"]), sc.N)
            delta, status = 0.0, 0
            for p in range(passes):
                twin = engine.weak_measure_estimate(sums[i, p], w[i, p], sc.FIRST_MS, int(r["edge"]), c0, spacing)
                got = folds[i, p]
                for name in ("e_minus", "e_prompt", "e_plus", "wn", "dd", "c0", "n_groups", "status"):
                    assert got[name] == twin[name], (passes, spacing, i, p, name, got[name], twin[name])        # bit for bit
                assert abs(float(got["cn0_dbhz"]) - float(twin["cn0_dbhz"])) <= 1e-9
                assert int(got["c0"]) == (c0 + wm.llround(float(got["dd"]) * wm.ONE)) % wm.CODE_MOD
                c0, delta, status = int(got["c0"]), delta + float(got["dd"]), status | int(got["status"])
            o = rec[i]
            print(f"{sc.MEASURE_IDS[k]} passes {passes} spacing 2^{spacing.bit_length() - 1} candidate {i}: dd {[round(float(f['dd']), 5) for f in folds[i]]} "
                  f"code phase {float(o['code_phase_samples']):.4f} cn0 {float(o['cn0_dbhz']):.2f} groups {int(o['n_groups'])}")
            assert (int(o["c0"]), float(o["delta_chips"]), float(o["dd_last"]), int(o["status"])) == (c0, delta, float(folds[i, -1]["dd"]), status)
            assert float(o["cn0_dbhz"]) == float(folds[i, -1]["cn0_dbhz"]) and float(o["code_phase_samples"]) == mm.code_phase_samples(c0, sc.N)
            assert (int(o["stream"]), int(o["sat_id"]), float(o["doppler_hz"]), float(o["carrier_phase"]), int(o["edge"]), int(o["reserved"])) == \
                (int(r["stream"]), int(r["sat_id"]), float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["edge"]), 0)
            assert int(o["n_groups"]) == mm.n_groups(n_ms, sc.FIRST_MS, int(r["edge"])) == groups and mm.first_head(sc.FIRST_MS, int(r["edge"])) == head
            assert int(o["status"]) == 0 and np.all(folds[i]["n_groups"] == groups)


@pytest.mark.parametrize("k", [k for k in ROWS if sc.MEASURE_ROWS[k][0] in (59, 60)], ids=lambda k: sc.MEASURE_IDS[k])
def test_short_rows_are_the_models_on_the_devices_input(engine_factory, k):
    n_ms = sc.MEASURE_ROWS[k][0]
    c = case(engine_factory, k)
    rec = c["runs"][(2, 1 << 39)][0]
    worst_c0 = worst_cn0 = 0.0
    for i, r in enumerate(c["refined"]):
        m = mm.measure(c["x"][int(r["stream"])], sc.chips_pm(int(r["sat_id"])), sc.FS, sc.N, float(r["doppler_hz"]), float(r["carrier_phase"]),
                       int(r["code_phase"]), int(r["edge"]), sc.FIRST_MS, n_ms)
        d_c0 = abs((int(rec[i]["c0"]) - m.c0 + wm.CODE_MOD // 2) % wm.CODE_MOD - wm.CODE_MOD // 2) / wm.ONE
        d_cn0 = abs(float(rec[i]["cn0_dbhz"]) - m.cn0_dbhz)
        worst_c0, worst_cn0 = max(worst_c0, d_c0), max(worst_cn0, d_cn0)
        assert d_c0 <= 1e-4 and d_cn0 <= 1e-3, (i, d_c0, d_cn0)
        assert abs(float(rec[i]["delta_chips"]) - m.delta_chips) <= 1e-4 and abs(float(rec[i]["dd_last"]) - m.dd_last) <= 1e-4
        assert (int(rec[i]["n_groups"]), int(rec[i]["status"])) == (m.n_groups, m.status)
    print(f"{sc.MEASURE_IDS[k]}: largest |device - model|: {worst_c0:.3g} chip, {worst_cn0:.3g} dB")
