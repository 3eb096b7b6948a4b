"""Every refused call of the weak-signal host path, with its return code and the text gyp_last_error gives:
gyp_correlate_grid_hybrid(_dev), gyp_acquire_weak(_dev), gyp_weak_bank_create / set_channel / drop_channel / set_state and
gyp_weak_track_block(_dev) -- and, for the code the weak bank shares with it, the 1-ms bank's gyp_bank_create / set_channel /
drop_channel and gyp_track_block(_dev).

One table (refused_calls), one row per condition: where an `if` tests several conditions, each has a row of its own, and where the
ORDER of two checks decides the text a row violates both.  The expected (code, text) pairs are tests/golden/weak_refusals.json,
recorded once from the library as it stood before these entry points' planning, bank skeleton and staging were gathered into shared
helpers; the test reads the file and never writes it.  Before every row the error text of the context the row reports on (and the
thread's text behind gyp_last_error(NULL)) is set to a sentinel by another refused call, so a row that returned a code without a text
of its own would show the sentinel.  The rows marked `silent` are the calls the library refuses with a code alone (a NULL context,
bank or result pointer): there the sentinel is what the golden file holds.

2.046 Msps, N = 2046, a 64 KiB device buffer, two-channel banks.  A refused call launches nothing.  Not in the table: refusals that
come from HIP itself (their text quotes the call expression), and gyp_acquire_weak's refusal of more than 2^31 - 1 cells, which its
device form makes behind the upload of at least 16385 streams' samples (the device form's row covers the check)."""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from gypsum_amd import _lib
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "weak_refusals.json"
FS, N = 2_046_000, 2046
INF, NAN = float("inf"), float("nan")
ONE_CHIP = 1 << 40
CODE_MOD = 1023 * ONE_CHIP


def _inits(*rows):
    """CHAN_INIT records from (stream, sat_id, doppler_hz, carrier_phase, code_phase) tuples."""
    r = np.zeros(len(rows), dtype=_lib.CHAN_INIT)
    for i, (stream, sat, dop, phase, code) in enumerate(rows):
        r[i] = (stream, sat, dop, phase, code, 0)
    return r


GOOD = ((0, 3, 1000.0, 0.5, 100), (1, 7, -2000.0, 1.5, 2000))      # channel 1 reads stream 1


def _params(**changes):
    r = np.zeros(1, dtype=_lib.WEAK_PARAMS)
    _lib.load().gyp_weak_params_default(_lib.ptr(r))
    r["sync_ms"] = 40
    for k, v in changes.items():
        r[k] = v
    return r


def _state(**changes):
    r = np.zeros(1, dtype=_lib.WEAK_STATE)
    r["f"], r["f_int"], r["u0"], r["c0"], r["edge"] = 100.0, 100.0, 0.5, 5, 3
    for k, v in changes.items():
        r[k] = v
    return r


class Env:
    """A context at 2.046 Msps with a 64 KiB device buffer, a weak bank and a 1-ms bank of two channels each (cursor 100), a second
    context that has no stream format, and 2 ms of host samples for the host forms whose refusal comes after the upload."""

    def __init__(self) -> None:
        self.eng = GypsumEngine(0)
        self.eng.set_stream_format(FS, N)
        self.bare = GypsumEngine(0)
        self.lib, self.ctx = self.eng.lib, self.eng.ctx
        self.buf = self.eng.alloc(1 << 16)
        self.p = self.buf.ptr.value
        self.host = np.zeros(8 * N, dtype=np.complex64)    # (2 streams x 2 ms at twice the rate: the row that uploads most)
        self.weak = self.eng.create_weak_bank(_inits(*GOOD), _params(), 100)
        self.bank = self.eng.create_bank(_inits(*GOOD))

    def close(self) -> None:
        self.weak.close()
        self.bank.close()
        self.buf.free()
        self.bare.close()
        self.eng.close()


def refused_calls(env: Env):
    """[(id, whose error text: a context's, or None for gyp_last_error(NULL)'s, silent, the call)]."""
    lib, ctx, bare, p = env.lib, env.ctx, env.bare.ctx, env.p
    ptr = _lib.ptr
    host = ptr(env.host)
    rows = []

    def row(name, call, where=ctx, silent=False):
        rows.append((name, where, silent, call))

    def ids(*v):
        return np.array(v, dtype=np.int32)

    def f64(*v):
        return np.array(v, dtype=np.float64)

    # ------------------------------------------------------------------------ gyp_correlate_grid_hybrid_dev / gyp_correlate_grid_hybrid
    def grid_dev(c=ctx, iq=p, ns=1, stride=N, T=1, blocks=1, flags=0, sats=ids(1), n_sats=None, bins=f64(0.0), n_bins=None, out=p):
        return lambda: lib.gyp_correlate_grid_hybrid_dev(c, iq, ns, stride, T, blocks, flags, ptr(sats), len(sats) if n_sats is None else n_sats,
                                                         ptr(bins), len(bins) if n_bins is None else n_bins, out)

    def grid_host(c=ctx, iq=host, ns=1, stride=None, T=1, blocks=1, flags=0, sats=ids(1), n_sats=None, bins=f64(0.0), n_bins=None, out=host):
        return lambda: lib.gyp_correlate_grid_hybrid(c, iq, ns, T, blocks, flags, ptr(sats), len(sats) if n_sats is None else n_sats,
                                                     ptr(bins), len(bins) if n_bins is None else n_bins, out)

    # ------------------------------------------------------------------------ gyp_acquire_weak_dev / gyp_acquire_weak
    def weak_dev(c=ctx, iq=p, ns=1, stride=N, T=1, blocks=1, flags=0, center=0.0, spread=500.0, step=0.0, sats=ids(1), n_sats=None, out=p):
        return lambda: lib.gyp_acquire_weak_dev(c, iq, ns, stride, T, blocks, flags, center, spread, step, ptr(sats),
                                                len(sats) if n_sats is None else n_sats, out)

    def weak_host(c=ctx, iq=host, ns=1, stride=None, T=1, blocks=1, flags=0, center=0.0, spread=500.0, step=0.0, sats=ids(1), n_sats=None, out=host):
        return lambda: lib.gyp_acquire_weak(c, iq, ns, T, blocks, flags, center, spread, step, ptr(sats), len(sats) if n_sats is None else n_sats, out)

    for name, call, dev in (("grid_dev", grid_dev, True), ("grid", grid_host, False), ("weak_dev", weak_dev, True), ("weak", weak_host, False)):
        is_grid = name.startswith("grid")
        row(f"{name}: ctx NULL", call(c=None), None, True)
        row(f"{name}: no stream format", call(c=bare), bare)
        row(f"{name}: no stream format and iq NULL", call(c=bare, iq=None), bare)
        row(f"{name}: iq NULL", call(iq=None))
        row(f"{name}: out NULL", call(out=None))
        row(f"{name}: sat ids NULL", call(sats=None, n_sats=1))
        row(f"{name}: n_streams 0", call(ns=0))
        row(f"{name}: n_sats 0", call(n_sats=0))
        if dev:
            row(f"{name}: stride -1", call(stride=-1))
        if is_grid:
            row(f"{name}: n_bins 0", call(n_bins=0))
            row(f"{name}: Doppler NULL", call(bins=None, n_bins=1))
            row(f"{name}: Doppler NULL and coherent_ms 0", call(bins=None, n_bins=1, T=0))
        row(f"{name}: coherent_ms 0", call(T=0))
        row(f"{name}: coherent_ms 21", call(T=21))
        row(f"{name}: n_blocks 0", call(blocks=0))
        row(f"{name}: n_blocks * coherent_ms 65536", call(T=16, blocks=4096))
        row(f"{name}: flag bit 4", call(blocks=2, flags=4))
        row(f"{name}: ALTERNATE with one block", call(flags=1))
        row(f"{name}: iq NULL and coherent_ms 0", call(iq=None, T=0))
        row(f"{name}: coherent_ms 0 and n_blocks 0", call(T=0, blocks=0))
        row(f"{name}: n_blocks 0 and flag bit 4", call(blocks=0, flags=4))
        row(f"{name}: flag bit 4 and ALTERNATE with one block", call(flags=5))
        row(f"{name}: satellite 0", call(sats=ids(1, 0)))
        row(f"{name}: satellite 33", call(sats=ids(33)))
        row(f"{name}: coherent_ms 21 and satellite 33", call(T=21, sats=ids(33)))
        if is_grid:
            row(f"{name}: Doppler inf", call(bins=f64(0.0, INF)))
            row(f"{name}: Doppler nan", call(bins=f64(NAN)))
            row(f"{name}: satellite 33 and Doppler nan", call(sats=ids(33), bins=f64(NAN)))
            row(f"{name}: 2^31 cells", call(ns=1 << 20, sats=ids(*range(1, 33)), bins=np.zeros(64)))
            if dev:
                row(f"{name}: Doppler nan and 2^31 cells", call(ns=1 << 20, sats=ids(*range(1, 33)), bins=f64(*([0.0] * 63 + [NAN]))))
        else:
            many = ids(*(list(range(1, 33)) + [1]))
            row(f"{name}: n_sats 33", call(sats=many))
            row(f"{name}: n_sats 33 and satellite 33", call(sats=ids(*range(1, 34))))
            row(f"{name}: n_sats 33 and centre nan", call(sats=many, center=NAN))
            row(f"{name}: centre nan", call(center=NAN))
            row(f"{name}: centre inf", call(center=INF))
            row(f"{name}: spread inf", call(spread=INF))
            row(f"{name}: spread nan", call(spread=NAN))
            row(f"{name}: step nan", call(step=NAN))
            row(f"{name}: step inf", call(step=-INF))
            row(f"{name}: spread 0", call(spread=0.0))
            row(f"{name}: spread -1", call(spread=-1.0))
            row(f"{name}: spread 0 and 4097 fine bins", call(spread=0.0, step=250.0 / 2048))
            # T = 1: coarse bins every 500 Hz over [-spread, spread); fine bins j * step for |j * step| <= 250
            row(f"{name}: 0 coarse bins", call(center=1e300, spread=1.0))
            row(f"{name}: 4096 coarse bins, 4097 fine", call(spread=1_024_000.0, step=250.0 / 2048))
            row(f"{name}: 4097 coarse bins", call(spread=1_024_250.0))
            row(f"{name}: 4097 fine bins", call(step=250.0 / 2048))
            if dev:
                row(f"{name}: 2^31 cells", call(ns=16385, sats=ids(*range(1, 33)), spread=1_024_000.0))
                row(f"{name}: 4097 coarse bins and 2^31 cells", call(ns=16385, sats=ids(*range(1, 33)), spread=1_024_250.0))

    # ------------------------------------------------------------------------ gyp_weak_bank_create
    def create(c=ctx, inits=_inits(*GOOD), n_chan=None, prm=_params(), first=0, out=True):
        def run():
            h = C.c_void_p()
            rc = lib.gyp_weak_bank_create(c, ptr(inits), (len(inits) if inits is not None else 2) if n_chan is None else n_chan, ptr(prm), first,
                                          C.byref(h) if out else None)
            assert not h.value
            return rc
        return run

    def init_with(**kw):
        a = _inits(*GOOD)
        for k, v in kw.items():
            a[k][1] = v
        return a
    row("weak_create: ctx NULL", create(c=None), None, True)
    row("weak_create: out NULL", create(out=False), ctx, True)
    row("weak_create: no stream format", create(c=bare), bare)
    row("weak_create: chans NULL", create(inits=None))
    row("weak_create: n_chan 0", create(n_chan=0))
    row("weak_create: first_ms -1", create(first=-1))
    row("weak_create: first_ms -1 and period_ms 10", create(first=-1, prm=_params(period_ms=10)))
    for name, prm in (("period_ms 19", _params(period_ms=19)), ("period_ms 21", _params(period_ms=21)), ("sync_ms 39", _params(sync_ms=39)),
                      ("sync_ms 2001", _params(sync_ms=2001)), ("spacing 0", _params(spacing=0)), ("spacing 2^40 + 1", _params(spacing=ONE_CHIP + 1)),
                      ("pll_bw_hz 0", _params(pll_bw_hz=0.0)), ("pll_bw_hz above 50", _params(pll_bw_hz=np.nextafter(50.0, 51.0))),
                      ("pll_bw_hz nan", _params(pll_bw_hz=NAN)), ("dll_bw_hz 0", _params(dll_bw_hz=0.0)),
                      ("dll_bw_hz above 10", _params(dll_bw_hz=np.nextafter(10.0, 11.0))), ("dll_bw_hz nan", _params(dll_bw_hz=NAN)),
                      ("lose_mu below 0", _params(lose_mu=-np.nextafter(0.0, 1.0))), ("lose_mu above 20", _params(lose_mu=np.nextafter(20.0, 21.0))),
                      ("lose_mu nan", _params(lose_mu=NAN)), ("period_ms 10 and sync_ms 39", _params(period_ms=10, sync_ms=39)),
                      ("sync_ms 39 and spacing 0", _params(sync_ms=39, spacing=0)), ("spacing 0 and pll_bw_hz 0", _params(spacing=0, pll_bw_hz=0.0)),
                      ("pll_bw_hz 0 and dll_bw_hz 0", _params(pll_bw_hz=0.0, dll_bw_hz=0.0)), ("dll_bw_hz 0 and lose_mu 21", _params(dll_bw_hz=0.0, lose_mu=21.0))):
        row(f"weak_create: {name}", create(prm=prm))
    weak_inits = (("stream -1", dict(stream=-1)), ("satellite 0", dict(sat_id=0)), ("satellite 33", dict(sat_id=33)), ("Doppler nan", dict(doppler_hz=NAN)),
                  ("Doppler inf", dict(doppler_hz=INF)), ("carrier phase nan", dict(carrier_phase=NAN)), ("carrier phase inf", dict(carrier_phase=-INF)),
                  ("stream -1 and satellite 0", dict(stream=-1, sat_id=0)), ("satellite 0 and Doppler nan", dict(sat_id=0, doppler_hz=NAN)),
                  ("Doppler nan and carrier phase nan", dict(doppler_hz=NAN, carrier_phase=NAN)))
    for name, kw in weak_inits:
        row(f"weak_create: {name}", create(inits=init_with(**kw)))
    row("weak_create: lose_mu 21 and satellite 0", create(prm=_params(lose_mu=21.0), inits=init_with(sat_id=0)))

    # ------------------------------------------------------------------------ gyp_weak_bank_set_channel / drop_channel / set_state
    wh, one = env.weak.handle, _inits(GOOD[0])
    row("weak_set_channel: bank NULL", lambda: lib.gyp_weak_bank_set_channel(None, 0, ptr(one)), ctx, True)
    row("weak_set_channel: index -1", lambda: lib.gyp_weak_bank_set_channel(wh, -1, ptr(one)))
    row("weak_set_channel: index n_chan", lambda: lib.gyp_weak_bank_set_channel(wh, 2, ptr(one)))
    row("weak_set_channel: init NULL", lambda: lib.gyp_weak_bank_set_channel(wh, 0, None))
    for name, kw in weak_inits:
        row(f"weak_set_channel: {name}", lambda a=init_with(**kw)[1:]: lib.gyp_weak_bank_set_channel(wh, 0, ptr(a)))
    row("weak_set_channel: index -1 and satellite 0", lambda a=init_with(sat_id=0)[1:]: lib.gyp_weak_bank_set_channel(wh, -1, ptr(a)))
    row("weak_drop_channel: bank NULL", lambda: lib.gyp_weak_bank_drop_channel(None, 0), ctx, True)
    row("weak_drop_channel: index -1", lambda: lib.gyp_weak_bank_drop_channel(wh, -1))
    row("weak_drop_channel: index n_chan", lambda: lib.gyp_weak_bank_drop_channel(wh, 2))
    row("weak_set_state: bank NULL", lambda: lib.gyp_weak_bank_set_state(None, 0, ptr(_state())), ctx, True)
    row("weak_set_state: index -1", lambda: lib.gyp_weak_bank_set_state(wh, -1, ptr(_state())))
    row("weak_set_state: index n_chan", lambda: lib.gyp_weak_bank_set_state(wh, 2, ptr(_state())))
    row("weak_set_state: state NULL", lambda: lib.gyp_weak_bank_set_state(wh, 0, None))
    for name, kw in (("f nan", dict(f=NAN)), ("f inf", dict(f=INF)), ("f_int nan", dict(f_int=NAN)), ("f_int inf", dict(f_int=-INF)),
                     ("u0 below 0", dict(u0=-np.nextafter(0.0, 1.0))), ("u0 1", dict(u0=1.0)), ("u0 nan", dict(u0=NAN)), ("c0 -1", dict(c0=-1)),
                     ("c0 1023 chips", dict(c0=CODE_MOD)), ("edge -1", dict(edge=-1)), ("edge 20", dict(edge=20))):
        row(f"weak_set_state: {name}", lambda s=_state(**kw): lib.gyp_weak_bank_set_state(wh, 0, ptr(s)))
    row("weak_set_state: index -1 and edge 20", lambda s=_state(edge=20): lib.gyp_weak_bank_set_state(wh, -1, ptr(s)))

    # ------------------------------------------------------------------------ gyp_weak_track_block_dev / gyp_weak_track_block
    def other_format(call):
        """The row's call under another stream format than the banks were created under; the format is put back behind it."""
        def run():
            assert lib.gyp_set_stream_format(ctx, 4_092_000, 4092) == 0
            rc = call()
            text = lib.gyp_last_error(ctx)
            assert lib.gyp_set_stream_format(ctx, FS, N) == 0      # (a call that succeeds leaves the error text as it is)
            assert lib.gyp_last_error(ctx) == text
            return rc
        return run

    def wtrack_dev(b=wh, iq=p, stride=2 * N, first=100, n_ms=2):
        return lambda: lib.gyp_weak_track_block_dev(b, iq, stride, first, n_ms, p, None, None)

    def wtrack(b=wh, iq=host, ns=2, first=100, n_ms=2):
        return lambda: lib.gyp_weak_track_block(b, iq, ns, first, n_ms, None, None, None)
    for name, call in (("weak_track_dev", wtrack_dev), ("weak_track", wtrack)):
        row(f"{name}: bank NULL", call(b=None), ctx, True)
        row(f"{name}: iq NULL", call(iq=None))
        row(f"{name}: n_ms 0", call(n_ms=0))
        row(f"{name}: n_ms 65536", call(n_ms=65536))
        row(f"{name}: iq NULL and n_ms 0", call(iq=None, n_ms=0))
        row(f"{name}: another stream format", other_format(call()))
        row(f"{name}: n_ms 0 and another stream format", other_format(call(n_ms=0)))
        row(f"{name}: first_ms 99", call(first=99))
        row(f"{name}: first_ms 101", call(first=101))
        row(f"{name}: another stream format and first_ms 99", other_format(call(first=99)))
    row("weak_track_dev: stride n_ms * N - 1", wtrack_dev(stride=2 * N - 1))
    row("weak_track_dev: first_ms 99 and stride n_ms * N - 1", wtrack_dev(first=99, stride=2 * N - 1))
    row("weak_track: n_streams 0", wtrack(ns=0))
    row("weak_track: n_streams 0 and iq NULL", wtrack(ns=0, iq=None))
    row("weak_track: a stream not passed", wtrack(ns=1))
    row("weak_track: first_ms 99 and a stream not passed", wtrack(ns=1, first=99))

    # ------------------------------------------------------------------------ the 1-ms bank
    def bcreate(c=ctx, inits=_inits(*GOOD), n_chan=None, out=True):
        def run():
            h = C.c_void_p()
            rc = lib.gyp_bank_create(c, ptr(inits), (len(inits) if inits is not None else 2) if n_chan is None else n_chan, C.byref(h) if out else None)
            assert not h.value
            return rc
        return run
    bh, t0 = env.bank.handle, np.zeros(2, dtype=np.float64)
    row("bank_create: ctx NULL", bcreate(c=None), None, True)
    row("bank_create: out NULL", bcreate(out=False), ctx, True)
    row("bank_create: no stream format", bcreate(c=bare), bare)
    row("bank_create: chans NULL", bcreate(inits=None))
    row("bank_create: n_chan 0", bcreate(n_chan=0))
    row("bank_create: stream -1", bcreate(inits=init_with(stream=-1)))
    row("bank_create: satellite 0", bcreate(inits=init_with(sat_id=0)))
    row("bank_create: satellite 33", bcreate(inits=init_with(sat_id=33)))
    row("bank_set_channel: bank NULL", lambda: lib.gyp_bank_set_channel(None, 0, ptr(one)), ctx, True)
    row("bank_set_channel: init NULL", lambda: lib.gyp_bank_set_channel(bh, 0, None))
    row("bank_set_channel: index -1", lambda: lib.gyp_bank_set_channel(bh, -1, ptr(one)))
    row("bank_set_channel: index n_chan", lambda: lib.gyp_bank_set_channel(bh, 2, ptr(one)))
    for name, kw in (("stream -1", dict(stream=-1)), ("satellite 0", dict(sat_id=0)), ("satellite 33", dict(sat_id=33))):
        row(f"bank_set_channel: {name}", lambda a=init_with(**kw)[1:]: lib.gyp_bank_set_channel(bh, 0, ptr(a)))
    row("bank_drop_channel: bank NULL", lambda: lib.gyp_bank_drop_channel(None, 0), ctx, True)
    row("bank_drop_channel: index -1", lambda: lib.gyp_bank_drop_channel(bh, -1))
    row("bank_drop_channel: index n_chan", lambda: lib.gyp_bank_drop_channel(bh, 2))

    def btrack_dev(b=bh, iq=p, n_ms=2, times=p):
        return lambda: lib.gyp_track_block_dev(b, iq, 2 * N, n_ms, times, None)

    def btrack(b=bh, iq=host, ns=2, n_ms=2, times=t0):
        return lambda: lib.gyp_track_block(b, iq, ns, n_ms, ptr(times), None)
    row("track_dev: bank NULL", btrack_dev(b=None), ctx, True)
    row("track_dev: iq NULL", btrack_dev(iq=None))
    row("track_dev: start times NULL", btrack_dev(times=None))
    row("track_dev: n_ms -1", btrack_dev(n_ms=-1))
    row("track_dev: another stream format", other_format(btrack_dev()))
    row("track_dev: n_ms -1 and another stream format", other_format(btrack_dev(n_ms=-1)))
    row("track_dev: n_ms 0 under another stream format", other_format(btrack_dev(n_ms=0)))
    row("track: bank NULL", btrack(b=None), ctx, True)
    row("track: iq NULL", btrack(iq=None))
    row("track: start times NULL", btrack(times=None))
    row("track: n_streams 0", btrack(ns=0))
    row("track: n_ms -1", btrack(n_ms=-1))
    row("track: a stream not passed", btrack(ns=1))
    row("track: n_ms -1 and a stream not passed", btrack(ns=1, n_ms=-1))
    row("track: a stream not passed, n_ms 0", btrack(ns=1, n_ms=0))
    row("track: another stream format", other_format(btrack()))
    return rows


NULL_SENTINEL = "gyp_create: out is NULL"


def run_table(env: Env):
    """{id: [code, text, the text before, silent]} of every row, each behind the sentinels."""
    lib, got = env.lib, {}
    for name, where, silent, call in refused_calls(env):
        for c in (env.ctx, env.bare.ctx):
            assert lib.gyp_debug_set(c, b"no_such_switch", 0.0) != 0
        assert lib.gyp_create(0, None) != 0 and lib.gyp_last_error(None).decode() == NULL_SENTINEL
        before = lib.gyp_last_error(where).decode()
        rc = call()
        text = lib.gyp_last_error(where).decode()
        assert name not in got, name
        got[name] = [int(rc), text, before, silent]
    return got


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def test_every_refusal_keeps_its_code_and_its_text(env):
    want = json.loads(GOLDEN.read_text())
    weak_before, bank_before = env.weak.state().tobytes(), {k: v.tobytes() for k, v in env.bank.state().items()}
    plan_before = env.eng.debug_get("last_hybrid_chunks")
    got = run_table(env)
    assert list(got) == list(want)                       # the same rows in the same order
    for name, (code, text, before, silent) in got.items():
        assert [code, text] == want[name], name
        assert code < 0, name
        if silent:
            assert text == before, name                  # a code alone
        else:
            assert text and text != before and text != NULL_SENTINEL, name      # refused, with a text of its own
    # a refused call changes nothing: the banks' states and cursor, the context's last hybrid plan
    assert env.weak.state().tobytes() == weak_before and env.weak.cursor == 100
    assert {k: v.tobytes() for k, v in env.bank.state().items()} == bank_before
    assert env.eng.debug_get("last_hybrid_chunks") == plan_before
    env.eng.sync()
