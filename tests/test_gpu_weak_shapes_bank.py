"""gyp_weak_track_block where its kernel's index arithmetic branches (the scene of tests/weak_shapes_scene.py): the edge step on SYNC
rows of 40, 47, 61 and 2000 prompts created at first_ms 0, 7 and 2^40 + 13 -- a sync_ms that is no multiple of 20, where the plan step
clips a chunk to what is left of SYNC; a sync_start that is no multiple of 20; the full sync_lds row -- against gyp_weak_bit_sync on
the device's own prompts, exactly: the same float64 + and x on the same float32 prompts; the phases SYNC -> WAIT -> TRACK that follow
from the edge; the same 92 ms in five calls; and banks of 8, 9, 13 and 17 channels, where the map from workgroups to channels is no
longer the identity, each channel against a one-channel bank.
"""
from __future__ import annotations

import numpy as np
import pytest

import weak_shapes_scene as sc
import weak_track_model as wm
from gypsum_amd import _lib, _records, engine

pytestmark = pytest.mark.gpu

_runs = {}


def run(engine_factory, sync_ms: int, first_ms: int, sizes=None):
    """Four channels on two streams through sync_ms + 45 milliseconds, in one call or in calls of `sizes`: (ms records, period
    records per channel, state).  The one-call runs are shared and left unchanged."""
    key = (sync_ms, first_ms, sizes)
    if key in _runs:
        return _runs[key]
    eng = engine_factory(sc.FS, sc.N)
    n_ms = sync_ms + sc.BANK_AFTER_MS
    x = sc.refine_iq()
    bank = eng.create_weak_bank(sc.inits_of(sc.refine_results()), _records.WeakParams(sync_ms=sync_ms), first_ms)
    try:
        at, ms_parts, per = 0, [], [[] for _ in range(4)]
        for step in sizes or (n_ms,):
            ms, pp = bank.track_block(sc.head_of(x, step, at), 2, first_ms + at, step)
            ms_parts.append(ms)
            for c in range(4):
                per[c].append(pp[c])
            at += step
        assert at == n_ms and bank.cursor == first_ms + n_ms
        state = bank.state()
    finally:
        bank.close()
    _runs[key] = (np.concatenate(ms_parts, axis=1), [np.concatenate(p) for p in per], state)
    return _runs[key]


@pytest.mark.parametrize("first_ms", sc.BANK_FIRST_MS)
@pytest.mark.parametrize("sync_ms", sc.SYNC_MS)
def test_edge_is_the_twins_on_the_devices_prompts_and_the_phases_follow(engine_factory, sync_ms, first_ms):
    n_ms = sync_ms + sc.BANK_AFTER_MS
    ms, per, state = run(engine_factory, sync_ms, first_ms)
    assert ms.shape == (4, n_ms) and np.all(ms["status"] == 0) and np.all(state["status"] == 0)
    for c in range(4):
        prompts = (ms[c, :sync_ms]["prompt_re"] + 1j * ms[c, :sync_ms]["prompt_im"]).astype(np.complex64)
        assert np.count_nonzero(prompts) == sync_ms
        en, edge = engine.weak_bit_sync(prompts, first_ms)
        order = np.sort(en)
        print(f"sync_ms {sync_ms} first_ms {first_ms} channel {c}: edge {int(state[c]['edge'])} (twin {edge}, scene {sc.refine_true_edge(c, first_ms)}), "
              f"largest energy over the second {order[-1] / order[-2]:.4f}")
        assert int(state[c]["edge"]) == edge                  # exact: no margin needed
        phase, pos, start = sc.expected_phases(first_ms, sync_ms, edge, n_ms)
        assert np.array_equal(ms[c]["phase"], phase) and np.array_equal(ms[c]["pos"], pos), (c, start)
        k = (n_ms - start) // 20
        assert k >= 1 and len(per[c]) == k
        assert int(per[c]["first_ms"][0]) == first_ms + start and np.all(np.diff(per[c]["first_ms"]) == 20) and np.all(per[c]["status"] == 0)
        assert (int(state[c]["phase"]), int(state[c]["pos"]), int(state[c]["n_periods"])) == (wm.TRACK, (n_ms - start) % 20, k)


@pytest.mark.parametrize("first_ms", sc.BANK_FIRST_MS)
def test_a_sync_of_47_does_not_depend_on_how_the_call_is_split(engine_factory, first_ms):
    one, parts = run(engine_factory, 47, first_ms), run(engine_factory, 47, first_ms, sc.SPLIT_47)
    assert parts[0].tobytes() == one[0].tobytes()
    for c in range(4):
        assert parts[1][c].tobytes() == one[1][c].tobytes(), c
    assert parts[2].tobytes() == one[2].tobytes()


# ---------------------------------------------------------------------------------------------- the channel map
_singles = {}


def bank_run(eng, inits: np.ndarray):
    """The scene's first 60 ms through a bank of these channels, by the device form into zeroed arrays: a row that no workgroup wrote
    stays zero and fails the comparison (the host form copies each channel's period records by the count the device left).
    (ms records [n, 60], period rows [n, 4], period counts [n], state [n])."""
    size, n_ms = len(inits), 60
    x = sc.head_of(sc.refine_iq(), n_ms)
    bank = eng.create_weak_bank(inits, _records.WeakParams(sync_ms=40), sc.FIRST_MS)
    mp = bank.max_periods(n_ms)
    d_iq = eng.alloc(x.nbytes).upload(x.reshape(-1))
    outs = [eng.alloc(nbytes).upload(np.zeros(nbytes, dtype=np.uint8))
            for nbytes in (size * n_ms * _lib.WEAK_MS_REC.itemsize, size * mp * _lib.WEAK_PERIOD_REC.itemsize, size * 4)]
    try:
        bank.track_block_dev(d_iq.ptr.value, n_ms * sc.N, sc.FIRST_MS, n_ms, outs[0].ptr.value, outs[1].ptr.value, outs[2].ptr.value)
        eng.sync()
        return (outs[0].download(_lib.WEAK_MS_REC, size * n_ms).reshape(size, n_ms), outs[1].download(_lib.WEAK_PERIOD_REC, size * mp).reshape(size, mp),
                outs[2].download(np.int32, size), bank.state())
    finally:
        for b in [d_iq] + outs:
            b.free()
        bank.close()


def single(eng, i: int):
    """Channel i of sc.bank_inits(...) alone in a bank (every size's inits are a head of the longest's)."""
    if i not in _singles:
        _singles[i] = bank_run(eng, sc.bank_inits(max(sc.BANK_SIZES))[i:i + 1])
    return _singles[i]


@pytest.mark.parametrize("size", sc.BANK_SIZES)
def test_every_channel_of_a_large_bank_is_the_one_channel_banks(engine_factory, size):
    eng = engine_factory(sc.FS, sc.N)
    inits = sc.bank_inits(size)
    assert inits.tobytes() == sc.bank_inits(max(sc.BANK_SIZES))[:size].tobytes()
    ms, per, cnt, state = bank_run(eng, inits)
    assert np.all(ms["status"] == 0) and np.all(ms["phase"][:, :40] == wm.SYNC) and np.all(ms["phase"][:, -1] == wm.TRACK)
    for i in range(size):
        one_ms, one_per, one_cnt, one_state = single(eng, i)
        assert ms[i].tobytes() == one_ms[0].tobytes(), (size, i)
        assert int(cnt[i]) == int(one_cnt[0]) and per[i].tobytes() == one_per[0].tobytes(), (size, i)
        assert state[i].tobytes() == one_state[0].tobytes(), (size, i)
        assert int(state[i]["phase"]) == wm.TRACK and int(state[i]["status"]) == 0
    assert len({ms[i].tobytes() for i in range(size)}) == size          # no two channels alike: a record in the wrong row would show
