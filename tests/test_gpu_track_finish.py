"""The throughput tracking kernel finishes a millisecond's profile only on the wavefronts that use it (gyp_debug_set
"track_finish_all").

At the single-round rates (up to 8 samples per chip) every wavefront publishes its candidate for the profile maximum; by default
wavefront 0 and the record wavefront then merge the candidates in straight-line code (one candidate per lane, a row reduction), the
code-loop wavefront reads its two taps and the others do nothing.  With "track_finish_all" 1 every thread walks the candidates for
itself again, in the chain of scalar branches the kernel had before.  Both forms must leave the same bytes everywhere: the same bank
is advanced from the same fresh state under 0 and under 1, and the records (field by field), the state read-back and the repair
counts of the exact code loop are compared.  Nothing here is compared with the oracle: the surveys do that for the default form.

Workgroup shapes: 8 wavefronts at 8.184 Msps, 4 at 4.092, 2 at 2.046 (code loop on wavefront 1, record fields on wavefront 0), 1 at
1.023 (every role on wavefront 0); 3, 5 and 6 wavefronts (3.069, 5.115, 6.138 Msps) leave lanes of the row reduction without a
candidate; 16.368 Msps runs two rounds and does not look at the switch.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from gypsum_amd import _lib, synth
from oracle import gypsum_oracle as orc

RATES = [8, 4, 2, 1, 3, 5, 6, 16]
N_STREAMS, SATS_PER_STREAM, N_MS = 2, 6, 40


@functools.lru_cache(maxsize=None)
def _inputs(k, zero_stream=False):
    """(streams, inits, t0): 2 streams x 6 satellites x 40 ms at rate k, a channel on every satellite a few Hz off its Doppler."""
    fs, n = 1_023_000 * k, 1023 * k
    scenes = [synth.random_scene(fs, N_MS, SATS_PER_STREAM, 730000 + 10 * k + b, max_code_phase=(2046 if n > 2046 else None))
              for b in range(N_STREAMS)]
    streams = [synth.render(s) for s in scenes]
    if zero_stream:
        streams[0] = np.zeros_like(streams[0])
    rng = np.random.default_rng(730000 + k)
    inits = np.zeros(N_STREAMS * SATS_PER_STREAM, dtype=_lib.CHAN_INIT)
    at = 0
    for b, s in enumerate(scenes):
        for sat in s.sats:
            inits[at] = (b, sat.sat_id, float(round(sat.doppler_hz)) + float(rng.integers(-2, 3)), float(sat.carrier_phase), sat.code_phase, 0)
            at += 1
    t0 = np.array([orc.chunk_times(ms * n, n, fs)[0] for ms in range(N_MS)])
    for s in streams:
        s.setflags(write=False)
    return streams, inits, t0


@pytest.fixture(scope="module")
def throughput_engine():
    """GypsumEngine per rate with the speculative tracker off: these small banks then run on the throughput kernel."""
    from gypsum_amd.engine import GypsumEngine

    cache = {}

    def make(k):
        if k not in cache:
            eng = GypsumEngine(0)
            eng.set_stream_format(1_023_000 * k, 1023 * k)
            eng.debug_set("no_spec", 1)
            cache[k] = eng
        return cache[k]

    yield make
    for eng in cache.values():
        eng.close()


def _run(eng, finish_all, k, streams, inits, t0, cuts, records=None, drop=None, reseed=None, keep=0):
    """A fresh bank advanced through `cuts` (ms per call).  records[i]: whether call i asks for records; drop: a channel dropped before
    the first call; reseed: (call index, channel, init) re-seeded before that call; keep: trailing profiles kept (the instrumented
    instantiation of the kernel).  Returns everything the two forms are compared on."""
    n = 1023 * k
    records = records or [True] * len(cuts)
    eng.debug_set("track_finish_all", finish_all)
    try:
        assert eng.debug_get("track_finish_all") == finish_all
        bank = eng.create_bank(inits)
        if keep:
            bank.keep_profiles(keep)
        if drop is not None:
            bank.drop_channel(drop)
        out = {"rec": [], "repairs": [], "state": []}
        at = 0
        for i, n_ms in enumerate(cuts):
            if reseed is not None and reseed[0] == i:
                bank.set_channel(reseed[1], reseed[2])
            seg = np.concatenate([s[at * n:(at + n_ms) * n] for s in streams])
            rec = bank.track_block(seg, len(streams), n_ms, t0[at:at + n_ms], want_records=records[i])
            out["rec"].append(rec)
            out["repairs"].append(bank.dll_repairs())
            out["state"].append(bank.state())
            at += n_ms
        if keep:
            out["profiles"] = [bank.profiles(ch) for ch in range(len(inits))]
        bank.close()
    finally:
        eng.debug_set("track_finish_all", 0)
    return out


def _assert_same(a, b, where):
    for i, (ra, rb) in enumerate(zip(a["rec"], b["rec"])):
        assert (ra is None) == (rb is None), (where, i)
        if ra is not None:
            differ = [f for f in ra.dtype.names if ra[f].tobytes() != rb[f].tobytes()]
            assert not differ, (where, f"call {i}", differ)
    for i, (sa, sb) in enumerate(zip(a["state"], b["state"])):
        differ = [f for f in sa if sa[f].tobytes() != sb[f].tobytes()]
        assert not differ, (where, f"state after call {i}", differ)
    for i, (da, db) in enumerate(zip(a["repairs"], b["repairs"])):
        assert da.tobytes() == db.tobytes(), (where, f"dll_repairs after call {i}", da, db)
    for ch, (pa, pb) in enumerate(zip(a.get("profiles", []), b.get("profiles", []))):
        assert pa.shape == pb.shape and pa.tobytes() == pb.tobytes(), (where, f"profiles of channel {ch}")


def _throughput_records(out):
    """Every record of every call came from the transform path (no speculative fast path), and some channel was tracked."""
    recs = [r for r in out["rec"] if r is not None]
    return all(not np.any((r["path_info"] & 3) == 1) for r in recs) and any(np.any(r["status"] == 0) for r in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(N_MS,), (1, N_MS - 1)], ids=["one-call", "1+39"])
@pytest.mark.parametrize("k", RATES, ids=[f"K{k}" for k in RATES])
def test_both_finishes_leave_the_same_bytes(throughput_engine, k, cuts):
    """2 streams x 12 channels x 40 ms as one call and cut 1 + 39 (the first millisecond after a reset ends a launch on its own)."""
    eng = throughput_engine(k)
    streams, inits, t0 = _inputs(k)
    narrow = _run(eng, 0, k, streams, inits, t0, cuts)
    every = _run(eng, 1, k, streams, inits, t0, cuts)
    assert _throughput_records(narrow)
    _assert_same(narrow, every, (k, cuts))


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(N_MS,), (1, N_MS - 1)], ids=["one-call", "1+39"])
@pytest.mark.parametrize("k", RATES, ids=[f"K{k}" for k in RATES])
def test_exact_ties_on_an_all_zero_stream(throughput_engine, k, cuts):
    """Stream 0 all zeros: every lag of every wavefront ties at 0, so the winner is decided by the key alone, the count of equal maxima
    runs over all wavefronts and every partial sum is 0.  The two forms are compared with each other only."""
    eng = throughput_engine(k)
    streams, inits, t0 = _inputs(k, True)
    assert not np.any(streams[0]) and np.any(streams[1])
    narrow = _run(eng, 0, k, streams, inits, t0, cuts)
    every = _run(eng, 1, k, streams, inits, t0, cuts)
    _assert_same(narrow, every, (k, cuts))


@pytest.mark.gpu
@pytest.mark.parametrize("k", RATES, ids=[f"K{k}" for k in RATES])
def test_dropped_and_reseeded_channels(throughput_engine, k):
    """Channel 1 dropped before the first call (status-2 records throughout), channel 7 re-seeded on another satellite's parameters
    between the two calls of 20 ms."""
    eng = throughput_engine(k)
    streams, inits, t0 = _inputs(k)
    again = tuple(inits[9])
    again = (again[0], again[1], again[2] + 3.0, again[3], again[4], again[5])
    kw = dict(drop=1, reseed=(1, 7, again))
    narrow = _run(eng, 0, k, streams, inits, t0, (20, 20), **kw)
    every = _run(eng, 1, k, streams, inits, t0, (20, 20), **kw)
    assert _throughput_records(narrow)
    assert np.all(narrow["rec"][0]["status"][1] == 2) and np.all(narrow["rec"][1]["status"][1] == 2)
    assert narrow["rec"][1]["doppler_hz"][7].tobytes() != narrow["rec"][1]["doppler_hz"][9].tobytes()   # (3 Hz apart: not one channel twice)
    _assert_same(narrow, every, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", RATES, ids=[f"K{k}" for k in RATES])
def test_records_off_and_kept_profiles(throughput_engine, k):
    """A call without records (rec_out null: the record is assembled in LDS and dropped) followed by one with them -- whatever the
    first call left in the loop state shows in the second call's records; and the instrumented instantiation of the kernel (trailing
    profiles kept), whose profile rows must be the same too."""
    eng = throughput_engine(k)
    streams, inits, t0 = _inputs(k)
    narrow = _run(eng, 0, k, streams, inits, t0, (25, 15), records=[False, True])
    every = _run(eng, 1, k, streams, inits, t0, (25, 15), records=[False, True])
    assert narrow["rec"][0] is None and _throughput_records(narrow)
    _assert_same(narrow, every, (k, "records off"))
    narrow = _run(eng, 0, k, streams, inits, t0, (N_MS,), keep=4)
    every = _run(eng, 1, k, streams, inits, t0, (N_MS,), keep=4)
    assert len(narrow["profiles"]) == len(inits) and narrow["profiles"][0].shape == (4, 1023 * k)
    _assert_same(narrow, every, (k, "profiles kept"))


@pytest.mark.gpu
def test_plain_device_call_with_and_without_records(throughput_engine):
    """gyp_track_block_dev on device buffers, as the benchmark calls it, at 8.184 Msps: with a record buffer, and with none followed by
    a call with one."""
    k = 8
    n = 1023 * k
    eng = throughput_engine(k)
    streams, inits, t0 = _inputs(k)
    host = np.concatenate(streams)
    d_iq = eng.alloc(host.nbytes).upload(host)
    d_t0 = eng.alloc(t0.nbytes).upload(t0)
    d_rec = eng.alloc(len(inits) * N_MS * _lib.TRACK_REC.itemsize)
    got = {}
    try:
        for finish_all in (0, 1):
            eng.debug_set("track_finish_all", finish_all)
            for with_rec in (True, False):
                bank = eng.create_bank(inits)
                bank.track_block_dev(d_iq.ptr.value, N_MS * n, N_MS, d_t0.ptr.value, d_rec.ptr.value if with_rec else 0)
                if not with_rec:   # what the record-less call left shows in a second pass over the same block
                    bank.track_block_dev(d_iq.ptr.value, N_MS * n, N_MS, d_t0.ptr.value, d_rec.ptr.value)
                eng.sync()
                rec = d_rec.download(_lib.TRACK_REC, len(inits) * N_MS).reshape(len(inits), N_MS)
                got[(finish_all, with_rec)] = (rec, bank.state(), bank.dll_repairs())
                bank.close()
    finally:
        eng.debug_set("track_finish_all", 0)
        for d in (d_iq, d_t0, d_rec):
            d.free()
    for with_rec in (True, False):
        (ra, sa, da), (rb, sb, db) = got[(0, with_rec)], got[(1, with_rec)]
        assert not np.any((ra["path_info"] & 3) == 1) and np.any(ra["status"] == 0)
        assert not [f for f in ra.dtype.names if ra[f].tobytes() != rb[f].tobytes()], with_rec
        assert not [f for f in sa if sa[f].tobytes() != sb[f].tobytes()], with_rec
        assert da.tobytes() == db.tobytes(), with_rec


@pytest.mark.gpu
def test_switch_is_range_checked(throughput_engine):
    from gypsum_amd.engine import GypsumHipError

    eng = throughput_engine(8)
    assert eng.debug_get("track_finish_all") == 0
    for bad in (-1, 2, 0.5):
        with pytest.raises(GypsumHipError):
            eng.debug_set("track_finish_all", bad)
    assert eng.debug_get("track_finish_all") == 0
