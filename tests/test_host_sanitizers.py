"""The host C++ of libgypsum_hip (gypsum_hip.hip, ingest.hpp, bit_integrator.hpp, grid_plan.hpp, track_plan.hpp, acq_plan.hpp, resample_plan.hpp, cond_plan.hpp, hybrid_plan.hpp, weak_plan.hpp, dev_mem.hpp) under ASan + UBSan and under TSan.

tests/host_san/driver.cpp is one translation unit with the product and has its own main; tests/host_san_build.py compiles it twice
(about 37 s for both, side by side; cached by content afterwards).  Each scenario below is one fresh child process that can see no
GPU: this file writes its inputs, the program writes raw arrays, and they are compared with numpy / big-integer models or with what the
uninstrumented library returns through ctypes for the same calls.  A sanitizer report in this project's code is a bug.

Nothing here is loaded into python under a sanitizer and nothing touches a GPU: the programs carry their own runtime, the
environment is inherited as it is and only gains the variables below.
"""
from __future__ import annotations

import ctypes as C
import errno
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bits_scenarios
import host_san_build
from gypsum_amd import _lib
from gypsum_amd.build import find_hipcc

# measured: both programs build in 37 s side by side, the longest scenario with its model (resample-plan under TSan, 5 million rows)
# takes 24 s; x2 for a loaded machine, rounded up
pytestmark = pytest.mark.timeout(120)

ASAN, TSAN = "asan_ubsan", "tsan"
BOTH = [ASAN, TSAN]
REPORT_WORDS = ("AddressSanitizer", "LeakSanitizer", "ThreadSanitizer", "runtime error:")
N = 2046
DTYPES = {0: np.float32, 1: np.int8, 2: np.int16, 3: np.uint8}      # GYP_FMT_*
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def programs():
    try:
        find_hipcc()
    except RuntimeError as e:
        pytest.skip(f"hipcc not found: {e}")
    return {name: r["path"] for name, r in host_san_build.build().items()}


def run(programs, which: str, scenario: str, tmp_path: Path) -> Path:
    """One scenario in a fresh child process; returns the directory it wrote."""
    out = tmp_path / f"out_{which}"
    out.mkdir()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", TSAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("ASAN_OPTIONS", None)
    r = subprocess.run([str(programs[which]), scenario, str(tmp_path / "in"), str(out)], env=env, capture_output=True, text=True, timeout=60)
    for word in REPORT_WORDS:
        assert word not in r.stderr, f"{which} {scenario}:\n{r.stderr[-6000:]}"
    assert r.returncode == 0, f"{which} {scenario}: exit {r.returncode}\n{r.stderr[-3000:]}"
    assert r.stdout.splitlines()[0] == host_san_build.BANNER[which]
    return out


def indir(tmp_path: Path) -> Path:
    d = tmp_path / "in"
    d.mkdir()
    return d


def i64(rows) -> np.ndarray:
    return np.array(rows, dtype="<i8")


def blocks(out: Path, name: str = "blocks"):
    """The driver's block log: (tag, first_ms, n_ms, bytes) per block handed out."""
    meta = np.fromfile(out / f"{name}.i64", dtype="<i8").reshape(-1, 4)
    blob = np.fromfile(out / f"{name}.bin", dtype=np.uint8)
    ends = np.cumsum(meta[:, 3])
    assert ends[-1] == len(blob) if len(meta) else len(blob) == 0
    return [(int(t), int(f), int(n), blob[e - b:e]) for (t, f, n, b), e in zip(meta, ends)]


def test_driver_never_makes_a_context():
    text = host_san_build.DRIVER.read_text()
    assert "gyp_create(" not in text
    assert "LD_PRELOAD" not in text and "verify_asan_link_order" not in text


# ------------------------------------------------------------------------------------------------------------ ingest-host
def reader_sequence(total: int, block_ms: int, start: int = 0):
    return [(f, min(block_ms, total - f)) for f in range(start, total, block_ms)]


@pytest.mark.parametrize("which", BOTH)
def test_ingest_host(programs, tmp_path, which):
    d = indir(tmp_path)
    rng = np.random.default_rng(11)
    files = {}
    for fmt, dt in DTYPES.items():
        item = np.dtype(dt).itemsize
        for idx, n_bytes in enumerate([0, 1, 2 * N * item, (2 * N + 1) * item, (23 * 2 * N + 2 * N - 1) * item]):
            files[idx, fmt] = rng.integers(0, 256, n_bytes, dtype=np.uint8)
            files[idx, fmt].tofile(d / f"f{idx}_{fmt}.bin")
    cases = []
    for (idx, fmt), data in files.items():
        ms_bytes = 2 * N * np.dtype(DTYPES[fmt]).itemsize
        total = (len(data) - 1) // ms_bytes if len(data) else 0
        for block_ms in (1, 5):
            for depth in (3, 64):
                cases.append((idx, fmt, N, block_ms, depth, total // 2))
    i64(cases).tofile(d / "cases.i64")
    rates, firsts = (2_046_000, 8_184_000, 16_368_000, 49_104_000), (0, 1, 999, 12345, 3_599_000, 86_399_990)   # test_times_equal_python_round
    i64([(fs, f) for fs in rates for f in firsts]).tofile(d / "times.i64")

    out = run(programs, which, "ingest-host", tmp_path)
    want_blocks, want_info = [], []
    for c, (idx, fmt, _, block_ms, depth, mid) in enumerate(cases):
        data = files[idx, fmt]
        ms_bytes = 2 * N * np.dtype(DTYPES[fmt]).itemsize
        total = (len(data) - 1) // ms_bytes if len(data) else 0
        assert total == [0, 0, 0, 1, 23][idx]
        seq = [(4 * c, f, n) for f, n in reader_sequence(total, block_ms)] + [(4 * c, -1, 0)]
        seq += [(4 * c + 1, -1, 0)] * 2 + [(4 * c + 2, -1, 0)]
        after = reader_sequence(total, block_ms, mid)[:2]
        seq += [(4 * c + 3, f, n) for f, n in after] + [(4 * c + 3, -1, 0)] * (2 - len(after))
        want_blocks += [(t, f, n, data[f * ms_bytes:(f + n) * ms_bytes] if n else data[:0]) for t, f, n in seq]
        want_info += [total, -1, -1, -1, -1, -1, -1, -1 if fmt == 0 else 0]
    want_info += [-1, -1, 0, _lib.GYP_E_IO, -1, -1, -1, -1, -2, -1]
    got = blocks(out)
    assert [(t, f, n) for t, f, n, _ in got] == [(t, f, n) for t, f, n, _ in want_blocks]
    for (t, f, n, a), (_, _, _, b) in zip(got, want_blocks):
        assert np.array_equal(a, b), (t, f, n)
    assert np.fromfile(out / "info.i64", dtype="<i8").tolist() == want_info
    times = np.fromfile(out / "times.f64", dtype="<f8").reshape(-1, 2, 40)
    k = 0
    for fs in rates:
        n = fs // 1000
        for first in firsts:
            assert times[k, 0].tolist() == [round((first + i) * n / fs, 6) for i in range(40)]
            assert times[k, 1].tolist() == [round((first + i + 1) * n / fs, 6) for i in range(40)]
            k += 1


# ------------------------------------------------------------------------------------------------------------ ingest-races
@pytest.mark.parametrize("which", BOTH)
def test_ingest_races(programs, tmp_path, which):
    d = indir(tmp_path)
    rng = np.random.default_rng(12)
    ms_bytes = 2 * N * 4
    total = 300
    rec = rng.integers(0, 256, total * ms_bytes + 20, dtype=np.uint8)
    rec.tofile(d / "rec.bin")
    rec[:20 * ms_bytes + 4].tofile(d / "shrinks.bin")
    seeks = np.random.default_rng(2026).integers(0, total + 1, 200)
    i64(seeks).tofile(d / "seeks.i64")

    out = run(programs, which, "ingest-races", tmp_path)

    def one(tag, ms, block_ms, tot=total):
        return (tag, ms, min(block_ms, tot - ms)) if ms < tot else (tag, -1, 0)

    want = [one(1, (i * 37) % (total + 1), 200) for i in range(0, 60, 3)]
    want += [one(2, int(ms), 4) for ms in seeks]
    want += [(3, f, n) for f, n in reader_sequence(total, 16)] + [(3, -1, 0)]
    want += [(4, 0, 2), (4, 2, 2), (4, 4, 2), (5, 0, 2)]
    got = blocks(out)
    assert [(t, f, n) for t, f, n, _ in got] == want
    for t, f, n, data in got:      # every block handed out is the file's bytes
        assert np.array_equal(data, rec[f * ms_bytes:(f + n) * ms_bytes]), (t, f, n)
    assert np.fromfile(out / "info.i64", dtype="<i8").tolist() == [_lib.GYP_E_IO, _lib.GYP_E_IO]
    assert (out / "shrinks_error.txt").read_text().strip() == "gyp_ingest: read failed: " + os.strerror(errno.EIO)
    for who, block_ms in ((0, 5), (1, 3)):
        want = []
        for start in (0, 0, 100):
            want += [(6 + who, f, n) for f, n in reader_sequence(total, block_ms, start)] + [(6 + who, -1, 0)]
        got = blocks(out, f"thread{who}")
        assert [(t, f, n) for t, f, n, _ in got] == want
        for t, f, n, data in got:
            assert np.array_equal(data, rec[f * ms_bytes:(f + n) * ms_bytes]), (who, f, n)
    assert (out / "thread_errors.txt").read_text().splitlines() == ["gyp_ingest_seek: millisecond out of range",
                                                                     "gyp_ingest_set_scale: scale must be positive and finite"]


# ------------------------------------------------------------------------------------------------------------ bits
def bits_plan():
    names = sorted(bits_scenarios.scenarios())
    # every stream in pushes of 1, 7 and 1000 symbols; capacities 0, 1 and ample crossed with 7 and 1000, in turn with 1 (a third of the calls)
    return names, [(k, push, cap, {0: 1, 1: 2, 4096: 0}[cap]) for k in range(len(names)) for push in (1, 7, 1000)
                   for cap in ((0, 1, 4096) if push > 1 else ((0, 1, 4096)[k % 3],))]


def block_table(streams):
    """3 channels x 1500 ms of gyp_track_rec: channel 1 loses lock at ms 700 (a status-1 record, status 2 after), channel 2 carries code phases."""
    n_ms = 1500
    recs = np.zeros((3, n_ms), dtype=_lib.TRACK_REC)
    for c, name in enumerate(("clean_phase7", "clean_phase0", "noisy15")):
        recs[c]["pseudosymbol"] = streams[name]["symbols"][:n_ms]
    recs[1, 700]["status"] = 1
    recs[1, 701:]["status"] = 2
    recs[1, 700:]["pseudosymbol"] = 0
    recs[2]["code_phase"] = (np.arange(n_ms) * 37) % 2046
    return recs, streams["clean_phase7"]["start"][:n_ms].copy(), streams["clean_phase7"]["end"][:n_ms].copy(), [0, 1, 20, 21, 100, 777, 1000, n_ms]


def bits_through_ctypes(streams, names, plan):
    """The driver's calls, one for one, on the uninstrumented library (pinned to the reference by test_bits.py)."""
    lib = _lib.load()
    events, cursors, states, counts = [], [], [], []

    def state(b, ch, into):
        st = np.zeros(1, dtype=_lib.BITS_STATE)
        assert lib.gyp_bits_get_state(b, ch, _lib.ptr(st)) == 0
        into.append(st.tobytes())

    for k, push, cap, reset in plan:
        s = streams[names[k]]
        sym, start, end = (np.ascontiguousarray(s[x]) for x in ("symbols", "start", "end"))
        b = C.c_void_p()
        assert lib.gyp_bits_create(3, C.byref(b)) == 0
        total, reset_done = len(sym), reset == 0
        ev = np.zeros(max(cap, 5), dtype=_lib.BIT_EVENT)
        cur = np.zeros(push, dtype=np.int32)
        n_ev = C.c_int32()
        for at in range(0, total, push):
            n = min(push, total - at)
            if not reset_done and at >= total // 2:
                assert lib.gyp_bits_reset(b, -1 if reset == 2 else 1) == 0
                reset_done = True
            ts, te = C.c_void_p(start.ctypes.data + 8 * at), C.c_void_p(end.ctypes.data + 8 * at)
            assert lib.gyp_bits_push(b, 1, n, ts, ts, te, C.c_void_p(sym.ctypes.data + at), _lib.ptr(cur), _lib.ptr(ev) if cap else None, cap, C.byref(n_ev)) == 0
            counts.append(n_ev.value)
            events.append(ev[:n_ev.value].tobytes())
            cursors.append(cur[:n].tobytes())
            state(b, 1, states)
        while True:
            assert lib.gyp_bits_drain(b, _lib.ptr(ev), 5, C.byref(n_ev)) == 0
            counts.append(n_ev.value)
            events.append(ev[:n_ev.value].tobytes())
            if n_ev.value == 0:
                break
        state(b, 0, states)
        lib.gyp_bits_destroy(b)
    recs, start, end, cuts = block_table(streams)
    b = C.c_void_p()
    assert lib.gyp_bits_create(3, C.byref(b)) == 0
    bev, bstates, bcounts = [], [], []
    n_ev = C.c_int32()
    for i, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
        cap = 3 if i % 2 else 1000
        ev = np.zeros(cap, dtype=_lib.BIT_EVENT)
        part = np.ascontiguousarray(recs[:, a:z])
        assert lib.gyp_bits_push_block(b, _lib.ptr(part), 3, z - a, _lib.ptr(np.ascontiguousarray(start[a:z])), _lib.ptr(np.ascontiguousarray(end[a:z])),
                                       _lib.ptr(ev), cap, C.byref(n_ev)) == 0
        bcounts.append(n_ev.value)
        bev.append(ev[:n_ev.value].tobytes())
        for c in range(3):
            state(b, c, bstates)
    lib.gyp_bits_destroy(b)
    return [b"".join(x) for x in (events, cursors, states, bev, bstates)] + [counts, bcounts]


def test_bits(programs, tmp_path):
    d = indir(tmp_path)
    streams = bits_scenarios.scenarios()
    names, plan = bits_plan()
    for k, name in enumerate(names):
        for key, ext in (("symbols", "sym"), ("start", "start"), ("end", "end")):
            np.ascontiguousarray(streams[name][key]).tofile(d / f"s{k}.{ext}")
    i64(plan).tofile(d / "plan.i64")
    recs, start, end, cuts = block_table(streams)
    recs.tofile(d / "recs.bin")
    start.tofile(d / "block.start")
    end.tofile(d / "block.end")
    i64(cuts).tofile(d / "cuts.i64")

    out = run(programs, ASAN, "bits", tmp_path)
    events, cursors, states, bev, bstates, counts, bcounts = bits_through_ctypes(streams, names, plan)
    assert sum(counts) > 2000 and sum(bcounts) > 100                        # the FIFO, the drain and the block path all emitted bits
    assert np.fromfile(out / "counts.i32", dtype="<i4").tolist() == counts
    assert np.fromfile(out / "block_counts.i32", dtype="<i4").tolist() == bcounts
    for name, want in (("events.bin", events), ("cursors.i32", cursors), ("states.bin", states), ("block_events.bin", bev), ("block_states.bin", bstates)):
        assert (out / name).read_bytes() == want, name
    lost = np.frombuffer(bstates, dtype=_lib.BITS_STATE).reshape(-1, 3)[-1]
    assert [int(v) for v in lost["processed_pseudosymbol_count"]] == [1500, 700, 1500]
    assert np.fromfile(out / "refusals.i64", dtype="<i8").tolist() == [-1] * 13


# ------------------------------------------------------------------------------------------------------------ spans
def span_model(bits, real, spm, file_bytes, first, n):
    """include/gypsum_hip.h's contract of gyp_packed_span in Python integers: (rc, in_first, in_n, first_byte, n_bytes, file_samples,
    total_ms, bit0); GYP_E_BAD_ARG, outputs untouched, where the contract's own arithmetic would leave int64."""
    bad = (-1,) + (-777,) * 7
    B = bits * (1 if real else 2)
    if n < 0 or file_bytes < 0 or spm < 1:
        return bad
    file_samples = 8 * file_bytes // B
    a, b = max(first, 0), min(first + n, file_samples)
    if not all(I64_MIN <= v <= I64_MAX for v in (8 * file_bytes, first + n)):
        return bad
    total_ms = (file_samples - 1) // spm if file_samples > 0 else 0
    if b <= a:                                       # no part inside the file: no byte arithmetic to do
        return (0, 0, 0, 0, 0, file_samples, total_ms, 0)
    if not all(I64_MIN <= v <= I64_MAX for v in (a * B, b * B + 7)):
        return bad
    first_byte = a * B // 8
    return (0, a, b - a, first_byte, (b * B + 7) // 8 - first_byte, file_samples, total_ms, a * B % 8)


def test_spans(programs, tmp_path):
    d = indir(tmp_path)
    cases, want = [], []
    for bits in (1, 2, 4):
        for real in (0, 1):
            for order in (0, 1):
                for file_bytes in (0, 1, 2, 4095, 4096, 2 ** 31, 2 ** 40, 2 ** 60):
                    fsamp = 8 * file_bytes // (bits * (1 if real else 2))
                    for first in (-2 ** 40, -1, 0, 1, fsamp - 1, fsamp, 2 ** 60):
                        for n in (0, 1, 7, 2 ** 31, 2 ** 60):
                            if first > I64_MAX:      # (the file_samples of a 2^60-byte file of 1-bit words: not an int64, cannot be asked)
                                continue
                            w = span_model(bits, real, N, file_bytes, first, n)
                            cases.append((bits, real, order, N, file_bytes, first, n, fsamp if w[0] == 0 else -1))
                            want.append(w)
    assert len(cases) > 3000 and sum(w[0] == 0 for w in want) > 2000 and sum(w[0] != 0 for w in want) > 100
    i64(cases).tofile(d / "cases.i64")
    out = run(programs, ASAN, "spans", tmp_path)
    pub = np.fromfile(out / "public.i64", dtype="<i8").reshape(-1, 8)
    stat = np.fromfile(out / "static.i64", dtype="<i8").reshape(-1, 5)
    for case, w, p, s in zip(cases, want, pub.tolist(), stat.tolist()):
        assert tuple(p) == w, case
        assert tuple(s) == ((w[1], w[2], w[3], w[4], w[7]) if w[0] == 0 else (0, 0, 0, 0, 0)), case
    assert len(pub) == len(stat) == len(cases)


# ------------------------------------------------------------------------------------------------------------ designs
def design_cases():
    """(kind, fs_in, fs_out, if_hz, taps, expected return code); kind 0 gyp_resample_design, 1 gyp_ddc_design."""
    from ddc_model import TAPS as DDC_TAPS
    from test_gpu_ddc import VALUE_CASES
    from test_gpu_resample_edges import EDGE_PAIRS, TAPS as RS_TAPS
    ok, arg, rate = 0, _lib.GYP_E_BAD_ARG, _lib.GYP_E_BAD_RATE
    rows = [(0, fi, fo, 0, t, ok) for fi, fo in EDGE_PAIRS for t in (0, *RS_TAPS)]
    rows += [(0, 2_048_000, 2_046_000, 0, t, arg) for t in (17, 96, 128, -16)]
    rows += [(0, 1_000_000, 2_000_000, 0, 16, ok), (0, 1_000_000, 2_001_000, 0, 16, rate),          # ratio 2 and one kHz past it
             (0, 4_000_000, 2_000_000, 0, 16, ok), (0, 4_001_000, 2_000_000, 0, 16, rate),          # ratio 0.5 and one kHz past it
             (0, 2_046_000, 2_046_000, 0, 32, rate), (0, 2_048_500, 2_046_000, 0, 32, rate), (0, 2_048_000, 2_046_500, 0, 32, rate),
             (0, 0, 2_046_000, 0, 32, rate), (0, 2_048_000, 0, 0, 32, rate), (0, -2_048_000, 2_046_000, 0, 32, rate)]
    rows += [(1, fi, fo, f, t, ok) for fi, fo, f in VALUE_CASES for t in (0, *DDC_TAPS)]
    rows += [(1, 16_368_000, 4_092_000, 4_092_000, t, arg) for t in (16, 24, 33, 256)]
    rows += [(1, 16_368_000, 2_046_000, 4_092_000, 128, ok), (1, 16_369_000, 2_046_000, 4_092_000, 128, rate),      # 8 fs_out >= fs_in
             (1, 16_368_000, 4_092_000, 1_841_400, 64, ok), (1, 16_368_000, 4_092_000, 1_841_399, 64, rate),        # 20 |if| >= 9 fs_out
             (1, 16_368_000, 4_092_000, -1_841_400, 64, ok), (1, 16_368_000, 4_092_000, -1_841_399, 64, rate),
             (1, 16_368_000, 4_092_000, 6_342_600, 64, ok), (1, 16_368_000, 4_092_000, 6_342_601, 64, rate),        # 20 |if| + 9 fs_out <= 10 fs_in
             (1, 16_368_000, 4_092_000, -6_342_600, 64, ok), (1, 16_368_000, 4_092_000, -6_342_601, 64, rate),
             (1, 16_368_000, 4_092_000, 0, 64, rate), (1, 2 ** 31, 2 ** 28, 2 ** 29, 64, rate), (1, 2_147_484_000, 268_436_000, 536_870_000, 64, rate),
             (1, 16_368_500, 4_092_000, 4_092_000, 64, rate), (1, 16_368_000, 4_092_500, 4_092_000, 64, rate),
             (1, 4_092_000, 8_184_000, 1_023_000, 64, rate), (1, 16_368_000, 4_092_000, 2 ** 40, 64, rate)]
    return rows


def test_designs(programs, tmp_path):
    d = indir(tmp_path)
    rows = design_cases()
    i64([r[:5] for r in rows]).tofile(d / "cases.i64")
    out = run(programs, ASAN, "designs", tmp_path)
    meta = np.fromfile(out / "meta.i64", dtype="<i8").reshape(-1, 3)
    tables = np.fromfile(out / "tables.f32", dtype=np.uint8)
    lib = _lib.load()
    at = 0
    for (kind, fi, fo, f, taps, want_rc), (rc, L, T) in zip(rows, meta.tolist()):
        assert rc == want_rc, (kind, fi, fo, f, taps)
        n_phases, t_out = C.c_int32(-1), C.c_int32(-1)
        if kind:
            assert lib.gyp_ddc_design(fi, fo, f, taps, None, C.byref(n_phases), C.byref(t_out)) == rc
        else:
            assert lib.gyp_resample_design(fi, fo, taps, None, C.byref(n_phases)) == rc
            t_out.value = (taps or 32) if rc == 0 else -1
        assert (L, T) == (n_phases.value, t_out.value)
        if rc:
            continue
        ref = np.zeros(L * T, dtype=np.float32)
        assert (lib.gyp_ddc_design(fi, fo, f, taps, _lib.ptr(ref), None, None) if kind else lib.gyp_resample_design(fi, fo, taps, _lib.ptr(ref), None)) == 0
        assert tables[at:at + 4 * L * T].tobytes() == ref.tobytes(), (kind, fi, fo, f, taps)
        at += 4 * L * T
    assert len(meta) == len(rows) and at == len(tables)


# ------------------------------------------------------------------------------------------------------------ misc
def test_misc(programs, tmp_path):
    d = indir(tmp_path)
    lib = _lib.load()
    cells = np.zeros(6, dtype=_lib.CELL)
    cells["peak"] = [1.5, 1.5, 2.0, 3.0, 0.0, 7.25]
    cells["n_max"] = [N, N, 3, 1, N, 1]
    cells["sum"] = [N * 1.5, 100.0, 6.0, 5000.0, 0.0, 7.25]          # 0/0, x/0, a zero mean, an ordinary profile, all zero, N - n_max = 0 below
    cells_n = np.array([N, N, N, N, N, 1], dtype="<i4")
    cells.tofile(d / "cells.bin")
    cells_n.tofile(d / "cells_n.i32")
    nav = [(seed, stream, sat, off, ms) for seed in (0, 1, 2 ** 63 + 5) for stream in (0, 3) for sat in (1, 32) for off in (0, 19)
           for ms in (-2 ** 40, -21, -20, -1, 0, 19, 20, 2 ** 40, 2 ** 40 + 19)]
    i64([tuple(v if v < 2 ** 63 else v - 2 ** 64 for v in row) for row in nav]).tofile(d / "nav.i64")
    n_list, sub_list = list(range(1, 3001)) + [10 ** 6], [100, 167, 500, 2000, 99, 2001, 0]
    i64(n_list + [-1] + sub_list).tofile(d / "layout.i64")      # (-1 closes the first list)

    out = run(programs, ASAN, "misc", tmp_path)
    chips = np.zeros(32 * 1023, dtype=np.uint8)
    assert lib.gyp_prn_chips(_lib.ptr(chips)) == 0
    assert (out / "prn_chips.u8").read_bytes() == chips.tobytes()
    lanes = np.fromfile(out / "lanes.f32", dtype=np.float32).reshape(2, -1)
    for row, sat in zip(lanes, (1, 32)):
        ref = np.zeros(32 * 64 * 2, dtype=np.float32)
        assert lib.gyp_prn_spectrum_lane_layout(sat, _lib.ptr(ref)) == 0
        assert row.tobytes() == ref.tobytes()
    assert np.fromfile(out / "lanes_rc.i64", dtype="<i8").tolist() == [0, 0, -1, -1, -1]
    with np.errstate(all="ignore"):
        pk = cells["peak"].astype(np.float64)
        want = pk / ((cells["sum"] - cells["n_max"] * pk) / (cells_n - cells["n_max"]).astype(np.float64))
    got = np.fromfile(out / "strength.f64", dtype="<f8")
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[0]) and got[1] == 0.0 and np.isinf(got[2])
    assert np.fromfile(out / "nav_bits.i64", dtype="<i8").tolist() == [lib.gyp_synth_nav_bit(*row) for row in nav]
    ref = np.zeros(1, dtype=_lib.PARAMS)
    lib.gyp_params_default(_lib.ptr(ref))
    assert (out / "params.f64").read_bytes() == ref.tobytes()
    layout = np.fromfile(out / "layout.i32", dtype="<i4").reshape(len(sub_list), len(n_list), 34)
    starts = np.zeros(33, dtype=np.int32)
    for s, sub in enumerate(sub_list):
        for i, n_ms in enumerate(n_list):
            starts[:] = -777
            n = lib.gyp_debug_spec_layout_for(n_ms, sub, _lib.ptr(starts))
            assert layout[s, i, 0] == n and np.array_equal(layout[s, i, 1:], starts), (n_ms, sub)
            if not 100 <= sub <= 2000:
                assert n == -1 and (starts == -777).all()
            else:
                assert 1 <= n <= 32 and starts[0] == 0 and starts[n] == n_ms and (np.diff(starts[:n + 1]) > 0).all() and (starts[n + 1:] == -777).all()
    null_rc = np.fromfile(out / "null_rc.i64", dtype="<i8").tolist()
    assert len(null_rc) > 60 and null_rc[:-1] == [-1] * (len(null_rc) - 1) and null_rc[-1] == 1


# ------------------------------------------------------------------------------------------------------------ halo-readers
def halo_cases():
    """(packed, fmt or bits, real, order, n_in, taps, block_ms, depth, file length in bytes) for the context-free handles of all four
    kinds: filtered words and filtered packed words at every tap count, and (taps 0: no halo, n_in = n) plain words and native packed words."""
    filtered, unfiltered = (16, 64, 128), (0,)
    kinds = [(0, fmt, real, 0, filtered) for fmt in DTYPES for real in (0, 1)]
    kinds += [(1, bits, real, (bits + real) % 2, filtered) for bits in (1, 2, 4) for real in (0, 1)]
    kinds += [(0, fmt, 0, 0, unfiltered) for fmt in DTYPES] + [(1, bits, 0, bits % 2, unfiltered) for bits in (1, 2, 4)]
    rows = []
    for packed, what, real, order, tap_counts in kinds:
        # bits per sample
        B = what * (1 if real else 2) if packed else 8 * np.dtype(DTYPES[what]).itemsize * (1 if real else 2)
        for n_in in (2048, 16368, 38192):
            for taps in tap_counts:
                lengths = [0, (taps // 4 * B + 7) // 8 + (1 if B > 8 else 0), ((n_in + 1) * B + 7) // 8, 23 * n_in * B // 8 + 5 * max(B // 8, 1) + (B // 16 or 1)]
                for block_ms in (1, 7):
                    rows += [(packed, what, real, order, n_in, taps, block_ms, 3, length) for length in lengths]
    return rows


@pytest.mark.parametrize("which", BOTH)
def test_halo_readers(programs, tmp_path, which):
    d = indir(tmp_path)
    rows = halo_cases()
    blob = np.random.default_rng(13).integers(0, 256, max(r[8] for r in rows), dtype=np.uint8)
    index = {length: i for i, length in enumerate(sorted({r[8] for r in rows}))}
    for length, i in index.items():
        blob[:length].tofile(d / f"h{i}.bin")
    cases = []
    for packed, what, real, order, n_in, taps, block_ms, depth, length in rows:
        B = what * (1 if real else 2) if packed else 8 * np.dtype(DTYPES[what]).itemsize * (1 if real else 2)
        file_samples = 8 * length // B
        total = (file_samples - 1) // n_in if packed else ((length - 1) // (n_in * B // 8) if length else 0)
        total = max(total, 0)
        cases.append((packed, what, real, order, n_in, taps, block_ms, depth, index[length], total // 2, B, file_samples, total, length))
    i64([c[:10] for c in cases]).tofile(d / "cases.i64")

    out = run(programs, which, "halo-readers", tmp_path)
    info = np.fromfile(out / "info.i64", dtype="<i8").reshape(-1, 3).tolist()
    got = blocks(out)
    spans = np.fromfile(out / "spans.i64", dtype="<i8").reshape(-1, 9).tolist()
    assert len(spans) == len(got)
    at = 0
    for c, (packed, what, real, order, n_in, taps, block_ms, depth, _, restart, B, file_samples, total, length) in enumerate(cases):
        halo_lo, halo_hi = (taps // 2 - 1, taps // 2) if taps else (0, 0)
        span = block_ms * n_in + halo_lo + halo_hi
        slot_bytes = (span * B + 7) // 8 + 1 if packed else span * B // 8
        assert info[c] == [total, file_samples, slot_bytes], cases[c]
        data = blob[:length]
        for tag, start in ((2 * c, 0), (2 * c + 1, restart)):
            for first, n_ms in reader_sequence(total, block_ms, start):
                t, f, n, raw = got[at]
                s0, count = first * n_in - halo_lo, n_ms * n_in + halo_lo + halo_hi
                # the span function's numbers: the window, its part [a, b) inside the file, the bytes covering that part, the zero-fill
                a, b = max(s0, 0), min(s0 + count, file_samples)
                inside = [a, b - a, a * B // 8, a * B % 8, (b * B + 7) // 8 - a * B // 8] if b > a else [0, 0, 0, 0, 0]
                pad_lo = 0 if packed else ((a - s0) if b > a else count) * B // 8
                pad_hi = 0 if packed else count * B // 8 - pad_lo - inside[4]
                assert spans[at] == [s0, count, *inside, pad_lo, pad_hi], (cases[c], first)
                assert len(raw) == pad_lo + inside[4] + pad_hi <= slot_bytes
                at += 1
                assert (t, f, n) == (tag, first, n_ms), cases[c]
                if packed:          # the covering bytes of the part inside the file, as they are in the file
                    rc, _, _, first_byte, n_bytes, _, _, _ = span_model(what, real, n_in, length, s0, count)
                    assert rc == 0
                    want = data[first_byte:first_byte + n_bytes]
                else:               # the zero-padded slice of the file's whole samples
                    sb = B // 8
                    want = np.zeros(count * sb, dtype=np.uint8)
                    a, b = max(s0, 0), min(s0 + count, file_samples)
                    if b > a:
                        want[(a - s0) * sb:(b - s0) * sb] = data[a * sb:b * sb]
                assert np.array_equal(raw, want), (cases[c], first)
    assert at == len(got)
    cols = np.array(spans)      # the cases reach: a halo before sample 0, one past the end, a part that starts inside a byte
    assert (cols[:, 7] > 0).any() and (cols[:, 8] > 0).any() and (cols[:, 5] != 0).any() and (cols[:, 0] < 0).any()


# ------------------------------------------------------------------------------------------------------------ small-parsers
def cpulist_model(text: str, setsize: int):
    """ingest.hpp parse_cpulist on digits, '-' and ',': stop at the first malformed item, clip at CPU_SETSIZE."""
    import re
    cpus, p = set(), 0
    while p < len(text):
        m = re.compile(r"\d+").match(text, p)
        if not m:
            break
        a = b = int(m.group())
        p = m.end()
        if text[p:p + 1] == "-":
            m = re.compile(r"\d+").match(text, p + 1)
            if not m or int(m.group()) < a:
                break
            b, p = int(m.group()), m.end()
        cpus.update(range(a, min(b, setsize - 1) + 1))
        if text[p:p + 1] != ",":
            break
        p += 1
    return cpus


def test_small_parsers(programs, tmp_path):
    d = indir(tmp_path)
    long_list = ",".join(f"{i}-{i + 1}" if i % 6 == 0 else str(i) for i in range(0, 2400, 3))
    assert len(long_list) >= 5000
    lists = ["0-31,128-159", "", "7", "3-1", "5,", "0-99999", "x", "1-", long_list, "0-3,9-8,12", "1023,1024,2", "4,,5"]
    (d / "cpulists.bin").write_bytes(b"".join(s.encode() + b"\0" for s in lists))
    (d / "empty").write_bytes(b"")
    (d / "big2000").write_bytes(b"7" * 1999 + b"\n")
    (d / "trailing").write_bytes(b"0-31,128-159 \n \n")
    rates, firsts = (2_046_000, 8_184_000, 16_368_000, 49_104_000), (0, 1, 999, 12345, 3_599_000, 86_399_990)
    xs = [(first + i) * (fs // 1000) / fs for fs in rates for first in firsts for i in range(41)] + [0.0, 1e-7, 86399.9999995]
    np.array(xs, dtype="<f8").tofile(d / "round6.f64")
    packs = np.zeros(12, dtype=_lib.PACKING)
    packs["bits"] = [1, 2, 4, 3, 0, 8, 2, 2, 2, 2, 2, 1]
    packs["real"] = [0, 1, 1, 0, 0, 0, 2, 0, 0, 0, 0, 1]
    packs["order"] = [0, 1, 0, 0, 0, 0, 0, 2, 0, 0, 0, 1]
    packs["reserved"] = [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    packs["levels"][9][3] = np.nan
    packs["levels"][10][0] = np.inf
    packs["levels"][11][2:] = np.nan                 # entries >= 2^bits are ignored
    packs.tofile(d / "packings.bin")

    out = run(programs, ASAN, "small-parsers", tmp_path)
    raw = (out / "cpusets.bin").read_bytes()
    setsize = int(np.frombuffer(raw[-4:], dtype="<i4")[0])
    sets = np.frombuffer(raw[:-4], dtype=np.uint8).reshape(len(lists), 1 + setsize)
    for text, row in zip(lists, sets):
        want = cpulist_model(text, setsize)
        assert set(np.flatnonzero(row[1:]).tolist()) == want and row[0] == (1 if want else 0), text[:40]
    assert cpulist_model("0-31,128-159", 1024) == set(range(32)) | set(range(128, 160)) and cpulist_model("1-", 1024) == set()
    raw = (out / "small_files.bin").read_bytes()
    got, at = [], 0
    while at < len(raw):
        n = int(np.frombuffer(raw[at:at + 8], dtype="<i8")[0])
        got.append(raw[at + 8:at + 8 + n])
        at += 8 + n
    assert got == [b"", b"", b"7" * 1999, b"0-31,128-159"]
    assert np.fromfile(out / "round6.f64", dtype="<f8").tolist() == [round(x, 6) for x in xs]
    bad_bits, levels = "packing.bits must be 1, 2 or 4", "packing.levels[c] must be finite for every code c < 2^bits"
    assert (out / "packings.txt").read_text().splitlines() == [
        "ok 1 0 0 2", "ok 2 1 1 2", "ok 4 1 0 4", bad_bits, bad_bits, bad_bits, "packing.real must be 0 or 1",
        "packing.order must be GYP_PACK_MSB_FIRST or GYP_PACK_LSB_FIRST", "packing.reserved must be 0", levels, levels, "ok 1 1 1 1", "packing is NULL"]


# ------------------------------------------------------------------------------------------------------------ grid-plan
RATES = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48)             # GYP_FOR_EACH_RATE
NO_PIPE, NO_SHARED_FWD, NO_GRID_FUSED, NO_GRID_PARTS = 1, 2, 4, 8   # the switches column of shapes.i64
# (k, n_units, n_sats, n_blk, switches, fused_waves, n_cus) -> (path, pipe, waves, gs, parts); None = not asserted.  gs is asserted on path 2 only.
PLAN_LITERALS = [
    ((2, 8192, 32, 1, 0, 12, 256), (1, None, 12, None, 1)),                      # cfg2
    ((2, 8192, 32, 1, NO_GRID_FUSED, 12, 256), (2, None, 12, 16, 2)),
    ((2, 4096, 32, 1, 0, 12, 256), (1, None, 12, None, 1)),                      # cfg4 on one GPU
    ((8, 4095, 32, 1, 0, 12, 256), (2, None, 12, 16, 4)),
    ((8, 4096, 32, 1, 0, 12, 256), (1, None, None, None, None)),
    ((8, 4320, 3, 1, 0, 12, 256), (2, None, 12, 4, 2)),
    ((48, 800, 32, 1, 0, 12, 256), (2, None, 12, 16, 48)),                       # cfg5
    ((48, 800, 32, 1, 0, 8, 256), (2, None, 8, 16, 24)),
    ((48, 800, 32, 1, NO_GRID_PARTS, 12, 256), (2, None, 12, 2, 1)),
    ((48, 800, 32, 1, 0, 12, 304), (2, None, 12, 16, 24)),
    ((1, 6, 11, 1, 0, 12, 256), (3, 0, None, None, None)),
    *[((k, 6, 11, 1, 0, 12, 256), (2, None, 12, 2, k)) for k in (5, 8, 16, 48)],
    ((48, 6, 11, 1, NO_GRID_PARTS, 12, 256), (3, 1, None, None, None)),
    ((2, 6, 1, 1, 0, 12, 256), (3, 1, None, None, None)),
    ((5, 6, 1, 1, 0, 12, 256), (3, 0, None, None, None)),
    ((2, 6, 4, 10, 0, 12, 256), (4, None, None, None, None)),
    ((8, 6, 11, 1, NO_PIPE, 12, 256), (3, 0, None, None, None)),
    ((16, 6, 11, 1, NO_PIPE, 12, 256), (4, None, None, None, None)),
    ((8, 8192, 32, 1, NO_SHARED_FWD, 12, 256), (3, 1, None, None, None)),
    ((3, 8192, 32, 1, NO_SHARED_FWD, 12, 256), (3, 0, None, None, None)),
    ((2, 8192, 33, 1, 0, 12, 256), (2, None, 12, 4, 1)),
]


def test_grid_plan(programs, tmp_path):
    """grid_plan (csrc/grid_plan.hpp) against tests/grid_plan_model.py on every combination of the axes below, and on the shapes whose
    plans are written out above."""
    import grid_plan_model

    d = indir(tmp_path)
    axes = [RATES, (64, 256, 304), (1, 2, 3, 6, 20, 255, 800, 3200, 4095, 4096, 4320, 8192, 100000), range(1, 34), (1, 2, 10), range(16), (8, 12)]
    sweep = np.stack([g.ravel() for g in np.meshgrid(*[np.array(a, dtype="<i8") for a in axes], indexing="ij")], axis=1)
    literal = i64([(k, cus, units, sats, blk, sw, fw) for (k, units, sats, blk, sw, fw, cus), _ in PLAN_LITERALS])
    shapes = np.concatenate([sweep, literal])
    assert len(sweep) == 12 * 3 * 13 * 33 * 3 * 16 * 2
    shapes.tofile(d / "shapes.i64")
    out = run(programs, ASAN, "grid-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(shapes), len(grid_plan_model.FIELDS))
    k, cus, units, sats, blk, sw, fw = shapes.T
    want = grid_plan_model.grid_plan(k, cus, units, sats, blk, sw & NO_PIPE, sw & NO_SHARED_FWD, sw & NO_GRID_FUSED, sw & NO_GRID_PARTS, fw)
    for col, field in enumerate(grid_plan_model.FIELDS):
        bad = np.flatnonzero(got[:, col] != want[field])
        assert len(bad) == 0, (field, len(bad), shapes[bad[0]].tolist(), int(got[bad[0], col]), int(want[field][bad[0]]))
    plans = {f: got[:, c] for c, f in enumerate(grid_plan_model.FIELDS)}
    assert np.array_equal(plans["folded_bytes"] == 0, plans["path"] == 1)
    assert set(np.unique(plans["path"])) == {1, 2, 3, 4}
    for row, (shape, expected) in zip(got[len(sweep):], PLAN_LITERALS):
        for field, value in zip(("path", "pipe", "waves", "gs", "parts"), expected):
            if value is not None:
                assert row[grid_plan_model.FIELDS.index(field)] == value, (shape, field, row.tolist())


# ------------------------------------------------------------------------------------------------------------ track-plan
T_NO_PIPE, T_NO_SPEC, T_SPEC_REDO, T_NO_EXACT_SHARED = 1, 2, 4, 8      # the switches column of the track-plan scenario's shapes.i64
# Read off the host code as it stood before track_plan.hpp, by hand: (k, n_cus, n_chan, n_ms, switches) with spec_sub_ms 0, track_chunk_ms 250,
# no kept profiles, kappa 20 -> {field: value}; "lengths" are the sub-blocks' lengths, "starts" their first milliseconds.
TRACK_LITERALS = [
    ((8, 256, 12, 1000, T_SPEC_REDO), {"flow": 3, "starts": [0, 242, 484, 726, 866, 951], "rounds": 10}),
    ((8, 256, 12, 2500, T_SPEC_REDO), {"flow": 3, "lengths": [488, 488, 488, 488, 280, 170, 98], "rounds": 11}),
    ((8, 256, 12, 200, T_SPEC_REDO), {"flow": 2, "n": 1}),
    ((8, 256, 25, 1000, T_SPEC_REDO), {"flow": 2, "n": 6}),
    ((8, 256, 12, 1000, T_SPEC_REDO | T_NO_SPEC), {"flow": 1, "chunk_ms": 250, "launches": 4, "exact_path": 2}),
    ((8, 256, 12, 1000, T_SPEC_REDO | T_NO_SPEC | T_NO_EXACT_SHARED), {"flow": 1, "chunk_ms": 250, "launches": 4, "exact_path": 1}),
    ((8, 256, 257, 1000, T_SPEC_REDO), {"flow": 1}),
    ((16, 256, 12, 1000, T_SPEC_REDO | T_NO_SPEC), {"flow": 1, "exact_path": 3}),
    *[((4, 256, 12, 1000, sw), {"flow": 1}) for sw in range(16)],
]


@pytest.mark.parametrize("which", BOTH)
def test_track_plan(programs, tmp_path, which):
    """track_plan (csrc/track_plan.hpp) against tests/track_plan_model.py on every combination of the axes below and on the shapes whose
    plans are written out above; the layout of every speculative row is also what gyp_debug_spec_layout_for returns."""
    import track_plan_model as model

    d = indir(tmp_path)
    # k, n_cus, n_chan, n_ms, keep_profiles, switches, spec_sub_ms, track_chunk_ms, kappa
    axes = [(1, 2, 4, 8, 16), (8, 256), (1, 12, 24, 25, 256, 257, 1536), (1, 19, 255, 256, 300, 1000, 2047, 2048, 2500, 12000), (0, 1), range(16),
            (0, 50, 100, 167, 500, 2000), (0, 20, 250), (0, 20)]
    sweep = np.stack([g.ravel() for g in np.meshgrid(*[np.array(a, dtype="<i8") for a in axes], indexing="ij")], axis=1)
    assert len(sweep) == 5 * 2 * 7 * 10 * 2 * 16 * 6 * 3 * 2
    literal = i64([(k, cus, chan, n_ms, 0, sw, 0, 250, 20) for (k, cus, chan, n_ms, sw), _ in TRACK_LITERALS])
    rows = np.concatenate([sweep, literal])
    k, cus, chan, n_ms, keep, sw, sub_ms, chunk, kappa = rows.T
    np.stack([k, 1023 * k, cus, chan, n_ms, keep, sw, sub_ms, chunk, kappa], axis=1).astype("<i8").tofile(d / "shapes.i64")
    out = run(programs, which, "track-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(rows), len(model.FIELDS))
    want = model.track_plans(k, 1023 * k, cus, chan, n_ms, keep, sw & T_NO_PIPE, sw & T_NO_SPEC, sw & T_SPEC_REDO, sub_ms, chunk, sw & T_NO_EXACT_SHARED, kappa)
    for col, field in enumerate(model.FIELDS):
        bad = np.flatnonzero(got[:, col] != want[:, col])
        assert len(bad) == 0, (field, len(bad), rows[bad[0]].tolist(), int(got[bad[0], col]), int(want[bad[0], col]))
    plans = {f: got[:, c] for c, f in enumerate(model.FIELDS)}
    assert set(np.unique(plans["flow"])) == {1, 2, 3} and set(np.unique(plans["exact_path"])) == {1, 2, 3}
    assert np.array_equal(plans["n"] == 0, plans["flow"] == 1) and np.array_equal(plans["rounds"] > 1, plans["flow"] == 3)
    assert (plans["launches"][plans["flow"] != 1] == 1).all() and plans["launches"].max() == 600
    # the library's own layout call, for every (block length, target sub-block length) a speculative row has
    lib = _lib.load()
    spec = plans["flow"] != 1
    target = np.where(sub_ms >= 100, sub_ms, np.where(k == 2, 167, 500))
    starts = np.zeros(33, dtype=np.int32)
    pairs = np.unique(np.stack([n_ms, target], axis=1)[spec], axis=0)
    assert len(pairs) == 10 * 4 + 1                  # (the sweep's, and the 200-ms block written out above)
    for block, sub in pairs.tolist():
        n = lib.gyp_debug_spec_layout_for(block, sub, _lib.ptr(starts))
        assert n >= 1
        same = got[spec & (n_ms == block) & (target == sub)]
        assert (same[:, 6] == n).all() and (same[:, 8:9 + n] == starts[:n + 1]).all() and (same[:, 9 + n:] == block).all(), (block, sub)
        assert (same[:, 7] == np.diff(starts[:n + 1]).max()).all(), (block, sub)
    for row, (shape, expected) in zip(got[len(sweep):], TRACK_LITERALS):
        plan = dict(zip(model.FIELDS, row.tolist()))
        first = [plan[f"start{i}"] for i in range(plan["n"] + 1)]
        plan["starts"], plan["lengths"] = first[:-1], np.diff(first).tolist()
        for field, value in expected.items():
            assert plan[field] == value, (shape, field, plan[field])


# ------------------------------------------------------------------------------------------------------------ acq-plan
A_NO_PIPE, A_NO_SHARED_FWD, A_NO_SPLIT, A_IS_HELPER = 1, 2, 4, 8      # the switches column of the acq-plan scenario's shapes.i64
# Read off the host code as it stood before acq_plan.hpp, by hand (acquire_search's level loop, `can_share`, the room formula and
# `spread * 4 >= acq_initial_spread_hz`; gyp_acquire_dev's `max(1, min(acq_lanes, n_streams / 2))` and `(n_streams - s0) / (lanes - i)`):
# (k, n_streams, n_sats, n_ms, switches, acq_lanes, single_level, spread0) with the default gyp_params -> {field: value}; "parts" are the
# parts' stream counts.  The two limits behind "fits" are new: cells are indexed in int32 (2^31 - 1 >= 28 n_streams n_sats) and
# acq_refine_kernel's grid has n_ms rows of blocks (65535 at the most).  2 739 137 streams x 28 satellites is the largest search of 28
# satellites that fits (2 147 483 408 cells; one stream more makes 2 147 484 192), so the round 2 739 000 x 28 (2 147 376 000) still does.
ACQ_LITERALS = [
    ((8, 1, 32, 10, 0, 2, 0, 7000.0), {"fits": 1, "n_levels": 10, "shared_levels": 3, "max_units": 84, "lanes": 1, "parts": [1]}),
    ((8, 13, 32, 10, 0, 2, 0, 7000.0), {"max_units": 819, "lanes": 2, "parts": [6, 7], "n_levels": 10, "shared_levels": 3}),      # the 1 GiB cap
    ((8, 13, 32, 10, 0, 4, 0, 7000.0), {"lanes": 4, "parts": [3, 3, 3, 4]}),
    ((8, 5, 32, 10, 0, 4, 0, 7000.0), {"lanes": 2, "parts": [2, 3]}),
    ((8, 4, 32, 40, 0, 2, 0, 7000.0), {"max_units": 204, "lanes": 2, "parts": [2, 2]}),
    ((8, 4, 32, 40, A_NO_SPLIT, 2, 0, 7000.0), {"max_units": 204, "lanes": 1, "parts": [4]}),
    ((8, 4, 32, 40, A_IS_HELPER, 2, 0, 7000.0), {"lanes": 1, "parts": [4]}),
    ((8, 1, 32, 8192, 0, 2, 0, 7000.0), {"max_units": 1, "shared_levels": 3}),
    ((8, 1, 32, 8193, 0, 2, 0, 7000.0), {"max_units": 0, "shared_levels": 0, "n_levels": 10, "spectra": 0}),
    ((4, 1, 32, 10, 0, 2, 0, 7000.0), {"max_units": 0, "shared_levels": 0, "n_levels": 10}),
    ((8, 1, 32, 10, A_NO_PIPE, 2, 0, 7000.0), {"max_units": 0, "shared_levels": 0, "n_levels": 10}),
    ((8, 1, 32, 10, A_NO_SHARED_FWD, 2, 0, 7000.0), {"max_units": 0, "shared_levels": 0}),
    ((8, 1, 32, 10, 0, 2, 1, 1750.0), {"n_levels": 1, "shared_levels": 1, "lanes": 1}),
    ((8, 1, 32, 10, 0, 2, 1, 1749.0), {"n_levels": 1, "shared_levels": 0}),
    ((8, 1, 32, 65535, 0, 2, 0, 7000.0), {"fits": 1, "refine_y": 65535}),
    ((8, 1, 32, 65536, 0, 2, 0, 7000.0), {"fits": 0, "n_levels": 0, "lanes": 0}),
    ((8, 2_739_000, 28, 10, 0, 2, 0, 7000.0), {"fits": 1, "n_cells": 2_147_376_000}),
    ((8, 2_739_137, 28, 10, 0, 2, 0, 7000.0), {"fits": 1, "n_cells": 2_147_483_408}),
    ((8, 2_739_138, 28, 10, 0, 2, 0, 7000.0), {"fits": 0, "n_cells": 0}),
    ((8, 2_739_000, 32, 10, 0, 2, 0, 7000.0), {"fits": 0}),
]


@pytest.mark.parametrize("which", BOTH)
def test_acq_plan(programs, tmp_path, which):
    """acq_plan (csrc/acq_plan.hpp) against tests/acq_plan_model.py on every combination of the axes below and on the searches whose
    plans are written out above."""
    import acq_plan_model as model

    d = indir(tmp_path)
    # k, n_streams, n_sats, n_ms, switches, acq_lanes, single_level, spread0, min_spread
    axes = [(1, 2, 4, 8, 16), (1, 2, 3, 4, 5, 13, 64), (1, 2, 31, 32), (1, 2, 10, 40, 8192, 8193, 65535, 65536), range(16), (1, 2, 3, 4), (0, 1),
            (7000.0, 1750.0, 1749.0, 10.0), (10.0, 437.5)]
    sweep = np.stack([g.ravel() for g in np.meshgrid(*[np.array(a, dtype=np.float64) for a in axes], indexing="ij")], axis=1)
    assert len(sweep) == 5 * 7 * 4 * 8 * 16 * 4 * 2 * 4 * 2
    literal = np.array([shape + (10.0,) for shape, _ in ACQ_LITERALS], dtype=np.float64)
    rows = np.concatenate([sweep, literal])
    k, streams, sats, n_ms, sw, lanes, single = rows[:, :7].astype(np.int64).T
    spread0, min_spread = rows[:, 7].copy(), rows[:, 8].copy()
    initial, bins = np.full(len(rows), 7000.0), np.full(len(rows), 10.0)
    shapes = np.stack([k, 1023 * k, streams, sats, n_ms, sw, lanes, single, *(x.view(np.int64) for x in (spread0, initial, min_spread, bins))], axis=1)
    shapes.astype("<i8").tofile(d / "shapes.i64")
    out = run(programs, which, "acq-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(rows), len(model.FIELDS))
    (d / "shapes.i64").unlink()                          # (a few hundred megabytes between them)
    (out / "plans.i64").unlink()
    want = model.acq_plans(k, 1023 * k, streams, sats, n_ms, spread0, single, initial, min_spread, bins, sw & A_NO_PIPE, sw & A_NO_SHARED_FWD,
                           sw & A_NO_SPLIT, sw & A_IS_HELPER, lanes)
    for col, field in enumerate(model.FIELDS):
        bad = np.flatnonzero(got[:, col] != want[:, col])
        assert len(bad) == 0, (field, len(bad), rows[bad[0]].tolist(), int(got[bad[0], col]), int(want[bad[0], col]))
    plans = {f: got[:, c] for c, f in enumerate(model.FIELDS)}
    fits = plans["fits"] == 1
    assert np.array_equal(fits[:len(sweep)], n_ms[:len(sweep)] <= 65535) and (got[~fits] == 0).all()      # (in the sweep the milliseconds alone decide)
    # levels: 7000 Hz down to 10 Hz 10 and to 437.5 Hz 5; 1750 and 1749 Hz down to 10 Hz 8, to 437.5 Hz 3 and 2 (437.25 is below); 10 Hz 1 and 0
    assert set(np.unique(plans["n_levels"][fits])) == {0, 1, 2, 3, 5, 8, 10} and set(np.unique(plans["shared_levels"])) == {0, 1, 3}
    assert set(np.unique(plans["lanes"][fits])) == {1, 2, 3, 4} and (plans["shared_levels"] <= plans["n_levels"]).all()
    total = sum(plans[f"lane_streams{i}"] for i in range(model.MAX_LANES))
    assert np.array_equal(total[fits], streams[fits]) and (plans["lane_streams0"][fits] >= np.minimum(streams[fits], 2)).all()
    assert np.array_equal(plans["shared_levels"] > 0, fits & (plans["max_units"] > 0) & (spread0 * 4.0 >= 7000.0) & ((single == 1) | (spread0 >= min_spread)))
    for row, (shape, expected) in zip(got[len(sweep):], ACQ_LITERALS):
        plan = dict(zip(model.FIELDS, row.tolist()))
        plan["parts"] = [plan[f"lane_streams{i}"] for i in range(plan["lanes"])]
        for field, value in expected.items():
            assert plan[field] == value, (shape, field, plan[field])


# ------------------------------------------------------------------------------------------------------------ resample-plan
RESAMPLE_TAPS, DDC_TAPS = (16, 24, 32, 48, 64), (32, 48, 64, 96, 128)
TILE_BUDGETS = (1016, 1024, 4088, 4096, 8184, 8192)          # "resample_tile_samples" at its ends and its default, and 8 less (packed words)
# Worked out by hand from resample_shape as it stood before resample_plan.hpp: (n_in kHz, n_out kHz, T, budget, n_ms, first_ms) ->
# (np_tile, pc_tile, n_pchunks, lds_samples, n_tiles, p_first, n_periods).  4000 -> 4092: g 4, L 1023, M 1000; 16368 -> 4092: g 4092,
# L 1, M 4; 38192 -> 8184: g 2728, L 3, M 14; 2048 -> 2046: g 2, L 1023, M 1024.
RESAMPLE_LITERALS = [
    ((4000, 4092, 32, 4096, 5, 3), (4, 1023, 1, 4031, 5, 12, 20)),
    ((4000, 4092, 32, 1024, 5, 3), (1, 1013, 2, 1024, 40, 12, 20)),
    ((4000, 4092, 32, 4088, 5, 3), (4, 1023, 1, 4031, 5, 12, 20)),       # the packed budget: the same plan as 4096
    ((4000, 4092, 32, 1031, 1, 0), (1, 1023, 1, 1031, 4, 0, 4)),         # M + T - 1: a whole period just fits
    ((4000, 4092, 32, 1030, 1, 0), (1, 1019, 2, 1030, 8, 0, 4)),         # one sample less: chunks
    ((16368, 4092, 64, 4096, 1, 0), (1008, 1, 1, 4095, 5, 0, 4092)),
    ((38192, 8184, 96, 4096, 2, 7), (285, 3, 1, 4085, 20, 19096, 5456)),
    ((2048, 2046, 16, 4096, 1, 0), (2, 1023, 1, 2063, 1, 0, 2)),
]
# the refusal's edges: (n_in, n_out, T, budget, n_ms, n_streams) -> (fits, n_tiles)
RESAMPLE_EDGES = [
    ((16368, 4092, 128, 1024, 117_555_312, 1), (1, 2_147_483_646)),
    ((16368, 4092, 128, 1024, 117_555_313, 1), (0, 0)),
    ((2048, 2046, 32, 4096, 1, 65535), (1, 1)),
    ((2048, 2046, 32, 4096, 1, 65536), (0, 0)),
]
MIXER_ROWS = [(16_368_000, 4_092_000), (16_368_000, -4_092_000), (16_368_000, -1), (38_192_000, -9_548_001), (2_147_483_000, -2_147_483_000),
              (5_000_000, -12_345_678), (1000, 0), (2_046_000, 2_046_000)]


def resample_sweep():
    """Rows (n_in, n_out, T, n_streams, first_ms, n_ms, budget): every stream rate; the resampler's input rates N_out/2 .. 2 N_out and
    the down-converter's N_out .. 8 N_out -- both ends, the neighbours of N_out and 61 rates in between, and at 1.023 and 2.046 Msps
    every kHz; every tap count; the six budgets and the two at the branch, M + T - 1 and M + T - 2; n_ms 1, 2, 9, 250 (first_ms goes
    with n_ms); n_streams 1, 2, 65535, 65536."""
    ms = np.array([(1, 0), (2, 7), (9, 3), (250, 1_000_000)])                   # (n_ms, first_ms)

    def cross(n_out, n_in, taps, streams):
        t, i = np.meshgrid(np.array(taps), n_in, indexing="ij")
        pairs = np.stack([i.ravel(), np.full(i.size, n_out), t.ravel()], axis=1).astype(np.int64)
        M = pairs[:, 0] // np.gcd(pairs[:, 0], pairs[:, 1])
        budgets = np.concatenate([np.broadcast_to(np.array(TILE_BUDGETS), (len(pairs), 6)), (M + pairs[:, 2] - 1)[:, None], (M + pairs[:, 2] - 2)[:, None]], axis=1)
        p, b, m, s = (x.ravel() for x in np.meshgrid(np.arange(len(pairs)), np.arange(8), np.arange(4), np.arange(len(streams)), indexing="ij"))
        return np.stack([pairs[p, 0], pairs[p, 1], pairs[p, 2], np.array(streams)[s], ms[m, 1], ms[m, 0], budgets[p, b]], axis=1)

    rows = []
    for k in RATES:
        n_out = 1023 * k
        for taps, lo, hi in ((RESAMPLE_TAPS, -(-n_out // 2), 2 * n_out), (DDC_TAPS, n_out, 8 * n_out)):
            allowed = lambda n_in: n_in[(n_in >= lo) & (n_in <= hi) & ((n_in != n_out) | (lo == n_out))]      # (the resampler refuses equal rates)
            some = np.unique(np.r_[np.linspace(lo, hi, 61).astype(np.int64), lo + 1, hi - 1, n_out - 1, n_out + 1, n_out + 2])
            rows.append(cross(n_out, allowed(some), taps, (1, 2, 65535, 65536)))
            if k <= 2:   # every kHz: the grid's height plays no part in the tiling, so these go with one stream
                rows.append(cross(n_out, allowed(np.setdiff1d(np.arange(lo, hi + 1), some)), taps, (1,)))
    return np.concatenate(rows)


@pytest.mark.parametrize("which", BOTH)
def test_resample_plan(programs, tmp_path, which):
    """resample_ratio and resample_tiling (csrc/resample_plan.hpp) against tests/resample_plan_model.py on the sweep above, the plans
    written out above, and for every plan that fits what makes it correct: the span resample_kernel stages for a tile (its own formula,
    model.tile_span) never exceeds the LDS reserved, on the first tile of every phase chunk and on the last (the widest: a tile holds
    np_tile periods, or fewer at the end), and the tiles cover [p_first, p_first + n_periods) x [0, L) exactly once.  mixer_params
    against Python integers."""
    import resample_plan_model as model

    d = indir(tmp_path)
    sweep = resample_sweep()
    literal = i64([(n_in, n_out, T, 1, first, n_ms, budget) for (n_in, n_out, T, budget, n_ms, first), _ in RESAMPLE_LITERALS])
    edges = i64([(n_in, n_out, T, n_streams, 0, n_ms, budget) for (n_in, n_out, T, budget, n_ms, n_streams), _ in RESAMPLE_EDGES])
    rows = np.concatenate([sweep, literal, edges])
    n_in, n_out, T, n_streams, first_ms, n_ms, budget = rows.T
    np.stack([n_in * 1000, n_out * 1000, T, n_streams, first_ms, n_ms, budget], axis=1).astype("<i8").tofile(d / "shapes.i64")
    i64(MIXER_ROWS).tofile(d / "mixers.i64")
    out = run(programs, which, "resample-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(rows), len(model.RATIO_FIELDS) + len(model.FIELDS))
    (d / "shapes.i64").unlink()
    (out / "plans.i64").unlink()
    ratio = model.resample_ratio(n_in * 1000, n_out * 1000)
    for col, field in enumerate(model.RATIO_FIELDS):
        assert np.array_equal(got[:, col], ratio[field]), field
    want = model.resample_tilings(n_in, n_out, T, n_streams, first_ms, n_ms, budget)
    tiling = got[:, len(model.RATIO_FIELDS):]
    for col, field in enumerate(model.FIELDS):
        bad = np.flatnonzero(tiling[:, col] != want[:, col])
        assert len(bad) == 0, (field, len(bad), rows[bad[0]].tolist(), int(tiling[bad[0], col]), int(want[bad[0], col]))
    plan = {f: tiling[:, c] for c, f in enumerate(model.FIELDS)}
    fits = plan["fits"] == 1
    assert np.array_equal(fits[:len(sweep)], n_streams[:len(sweep)] <= 65535) and (tiling[~fits] == 0).all()   # (in the sweep the streams alone decide)
    # the invariant, on every row that fits (none is excused)
    g, L, M = ratio["g"][fits], ratio["L"][fits], ratio["M"][fits]
    ok = {f: v[fits] for f, v in plan.items()}
    period_tiles = -(-ok["n_periods"] // ok["np_tile"])
    assert np.array_equal(ok["n_tiles"], period_tiles * ok["n_pchunks"])                       # one tile per (period tile, chunk)
    assert np.array_equal(ok["p_first"], first_ms[fits] * g) and np.array_equal(ok["n_periods"], n_ms[fits] * g)
    # np_tile periods a tile, the last one the rest: [p_first, p_first + n_periods) once; pc_tile phases a chunk, the last the rest: [0, L) once
    assert (ok["np_tile"] >= 1).all() and ((period_tiles - 1) * ok["np_tile"] < ok["n_periods"]).all()
    assert (ok["pc_tile"] >= 1).all() and ((ok["n_pchunks"] - 1) * ok["pc_tile"] < L).all() and (ok["n_pchunks"] * ok["pc_tile"] >= L).all()
    worst, taps = np.zeros(fits.sum(), dtype=np.int64), T[fits]
    has = np.arange(len(worst))                                                                 # the plans that have a chunk `chunk`
    for chunk in range(int(ok["n_pchunks"].max())):
        has = has[ok["n_pchunks"][has] > chunk]
        sub = {f: v[has] for f, v in ok.items()}
        for tile in (np.full(len(has), chunk), (period_tiles[has] - 1) * sub["n_pchunks"] + chunk):       # this chunk of the first and of the last period tile
            worst[has] = np.maximum(worst[has], model.tile_span(sub, L[has], M[has], taps[has], tile))
    over = np.flatnonzero(worst > ok["lds_samples"])
    assert len(over) == 0, (len(over), rows[fits][over[0]].tolist(), int(worst[over[0]]), int(ok["lds_samples"][over[0]]))
    assert (worst >= taps).all()
    assert {1, 2} <= set(np.unique(ok["n_pchunks"]).tolist()) and (ok["np_tile"] > 1).any()    # both branches were swept
    for row, (shape, expected) in zip(tiling[len(sweep):], RESAMPLE_LITERALS):
        p = dict(zip(model.FIELDS, row.tolist()))
        assert p["fits"] == 1 and (p["np_tile"], p["pc_tile"], p["n_pchunks"], p["lds_samples"], p["n_tiles"], p["p_first"], p["n_periods"]) == expected, (shape, p)
    for row, (shape, expected) in zip(tiling[len(sweep) + len(literal):], RESAMPLE_EDGES):
        assert (row[0], row[1]) == expected and (expected[0] or not row.any()), (shape, row.tolist())
    mixed = np.fromfile(out / "mixed.i64", dtype="<i8").reshape(len(MIXER_ROWS), 4)
    for (fs, f_hz), (got_fs, got_f, q_bits, y_bits) in zip(MIXER_ROWS, mixed.tolist()):
        f, q, y = model.mixer_params(fs, f_hz)
        assert got_fs == fs and got_f == f and 0 <= got_f < fs, (fs, f_hz, got_f)
        assert q_bits == np.float64(q).view(np.int64) and y_bits == np.float64(y).view(np.int64), (fs, f_hz)
        assert q == 4.0 / fs and y == 0.5 / fs


# ------------------------------------------------------------------------------------------------------------ cond-plan
# Worked out by hand from the launch functions as they stood before cond_plan.hpp (stats_launch, condition_launch, notch_launch,
# blank_launch, hist_launch, tones_launch, quality_launch, widen_launch, unpack_launch):
# (stage, n_cus, wg_per_cu, n, a, b, stride, in_addr, out_addr, flag) -> {field: value}.  256 CUs x 2 workgroups: a cap of 512.
def cond_literals():
    from cond_plan_model import BLANK, CONDITION, EXCISE, HIST, NOTCH, QUALITY, SPECTRUM, STATS, TONES, UNPACK, WIDEN
    big = 2 ** 31 + 5
    return [
        ((STATS, 256, 2, 2, 300, 0, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 512, "gy_first": 1, "items_first": 600, "ns_first": 2}),
        ((STATS, 256, 2, 1, 20, 0, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 20, "items_first": 20}),
        # one block of an ingest handle in place: 20 ms of 2046 samples as 20460 float4, 80 workgroups of 256 threads
        ((CONDITION, 256, 2, 1, 40920, 0, 0, 4096, 4096, 0), {"n_chunks": 1, "vec4": 1, "per_stream": 20460, "gx_first": 80, "gy_first": 1}),
        ((CONDITION, 256, 2, 1, 40920, 0, 0, 4096, 4104, 0), {"vec4": 0, "per_stream": 40920, "gx_first": 160}),
        ((CONDITION, 256, 2, 17, 2047, 0, 2049, 4096, 4096, 0), {"n_chunks": 3, "vec4": 0, "per_stream": 2047, "gx_first": 8, "gy_first": 8,
                                                                  "s0_last": 16, "ns_last": 1, "gx_last": 8, "gy_last": 1}),
        ((CONDITION, 256, 2, 17, big, 0, big + 1, 4096, 4096, 0), {"vec4": 1, "per_stream": 2 ** 30 + 3, "gx_first": 64, "gy_first": 8, "gx_last": 512, "gy_last": 1}),
        ((CONDITION, 1, 1, 8, 2047, 0, 2048, 0, 0, 0), {"n_chunks": 1, "cap": 1, "gx_first": 1, "gy_first": 8}),      # 1 / 8 workgroups: still one
        ((NOTCH, 256, 2, 1, 20, 2046, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 20, "items_first": 20, "lds_bytes": 16368}),
        ((NOTCH, 256, 2, 9, 250, 16384, 0, 0, 0, 0), {"n_chunks": 2, "gx_first": 512, "items_first": 2000, "gx_last": 250, "items_last": 250, "s0_last": 8,
                                                      "lds_bytes": 131072}),
        ((NOTCH, 256, 2, 1, 20, 16385, 0, 0, 0, 0), {"lds_bytes": 0, "gx_first": 20}),
        ((NOTCH, 256, 2, 1, 20, 2046, 0, 0, 0, 1), {"lds_bytes": 0, "gx_first": 20}),
        ((BLANK, 256, 2, 11, 1, 0, 0, 0, 0, 0), {"n_chunks": 2, "gx_first": 8, "gx_last": 3, "s0_last": 8, "ns_last": 3}),
        ((HIST, 256, 2, 1, 20460, 0, 0, 0, 0, 0), {"per_stream": 10230, "gx_first": 40, "gy_first": 1}),
        ((HIST, 256, 2, 9, 2046, 0, 0, 0, 0, 0), {"n_chunks": 2, "gx_first": 4, "gy_first": 8, "gx_last": 4, "gy_last": 1}),
        ((TONES, 256, 2, 1, 79, 257, 0, 0, 0, 0), {"n_chunks": 1, "cap": 2048, "items_first": 20303, "gx_first": 2048}),
        ((QUALITY, 256, 2, 2049, 1000, 20, 0, 0, 0, 0), {"n_chunks": 3, "per_stream": 50, "cap": 16384, "items_first": 51200, "gx_first": 12800,
                                                         "s0_last": 2048, "items_last": 50, "gx_last": 13}),
        ((QUALITY, 64, 2, 2049, 1000, 20, 0, 0, 0, 0), {"cap": 4096, "gx_first": 4096, "gx_last": 13}),
        ((WIDEN, 256, 2, 0, 81840, 0, 0, 0, 0, 0), {"gx_first": 21}),          # 5115 whole 16s: 20 workgroups, and the one more
        ((WIDEN, 256, 2, 0, 15, 0, 0, 0, 0, 0), {"gx_first": 1}),
        ((WIDEN, 256, 2, 0, 2 ** 32 + 7, 0, 0, 0, 0, 0), {"gx_first": 512}),
        ((UNPACK, 256, 2, 1, 40920, 2, 40920, 0, 4096, 0), {"items_first": 1279, "gx_first": 5, "vec4": 1}),
        ((UNPACK, 256, 2, 3, 40920, 2, 40921, 0, 4096, 0), {"items_first": 3837, "gx_first": 15, "vec4": 0}),
        # excise_launch's chunks of 8 streams, one workgroup per (stream, millisecond); spectrum_hist_launch's one launch of them all
        ((EXCISE, 256, 2, 11, 3, 0, 0, 0, 0, 0), {"n_chunks": 2, "gx_first": 24, "items_first": 24, "gx_last": 9, "items_last": 9, "s0_last": 8, "ns_last": 3}),
        ((EXCISE, 256, 2, 1, 1000, 0, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 512, "items_first": 1000}),
        ((SPECTRUM, 256, 2, 11, 3, 0, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 33, "items_first": 33, "ns_first": 11, "gy_first": 1}),
        ((SPECTRUM, 256, 2, 17, 250, 0, 0, 0, 0, 0), {"n_chunks": 1, "gx_first": 512, "items_first": 4250, "ns_first": 17}),
    ]


def cond_sweep():
    """Every stage over its own axes: 1, 64, 256, 304 CUs x 1, 2, 8 workgroups per CU; stream counts on both sides of 8 and 16 and the
    grid's height limit, channel counts on both sides of 1024 and 2048; odd and even strides; bases at offsets 0 and 8."""
    import cond_plan_model as m
    streams, chans = (1, 2, 7, 8, 9, 16, 17, 65535), (1, 1023, 1024, 1025, 2049)
    n_ms, n, big = (1, 3, 250, 10000), (1, 2, 1023, 16384, 16385, 49104, 65536), 2 ** 31 + 5
    rows = []
    for cus in (1, 64, 256, 304):
        for wg in (1, 2, 8):
            def add(stage, count, a, b=0, stride=0, in_addr=0, out_addr=0, flag=0):
                rows.append((stage, cus, wg, count, a, b, stride, in_addr, out_addr, flag))
            for s in streams:
                for ms in n_ms:
                    add(m.STATS, s, ms)
                    add(m.BLANK, s, ms)
                    add(m.EXCISE, s, ms)
                    add(m.SPECTRUM, s, ms)
                    for spm in n:
                        for no_lds in (0, 1):
                            add(m.NOTCH, s, ms, spm, flag=no_lds)
                for count in (0, 1, 2, 3, 2047, big):
                    for stride in (count | 1, (count + 2) & ~1):
                        for i in (0, 8):
                            for o in (0, 8):
                                add(m.CONDITION, s, count, stride=stride, in_addr=4096 + i, out_addr=8192 + o)
                for count in (1, 2, 3, 2046, big):
                    add(m.HIST, s, count)
                    for bits in (1, 2, 4):
                        for stride in (count | 1, (count + 2) & ~1):
                            for o in (0, 8):
                                add(m.UNPACK, s, count, bits, stride=stride, out_addr=8192 + o)
                if wg == 1:              # (their caps do not depend on it)
                    for n_blocks in (1, 3, 250):
                        for n_freq in (1, 8, 257):
                            add(m.TONES, s, n_blocks, n_freq)
            if wg == 1:
                for c in chans:
                    for ms in n_ms:
                        for window in (1, 20, 250, 10001):
                            add(m.QUALITY, c, ms, window)
            for words in (1, 15, 16, 17, 4095, 4096, 4097, 81840, 2 ** 32 + 7):
                add(m.WIDEN, 0, words)
    return i64(rows)


@pytest.mark.parametrize("which", BOTH)
def test_cond_plan(programs, tmp_path, which):
    """The plans of csrc/cond_plan.hpp against tests/cond_plan_model.py on the sweep above and on the shapes whose plans are written
    out above, and what makes a plan correct: its launches take the streams 0 .. n - 1 in order, each once, none more than K of
    them; every grid is at least 1 and at most its cap; a launch over rows is as high as it has streams; LDS stays within 128 KiB."""
    import cond_plan_model as m

    d = indir(tmp_path)
    sweep, literals = cond_sweep(), cond_literals()
    shapes = np.concatenate([sweep, i64([shape for shape, _ in literals])])
    shapes.tofile(d / "shapes.i64")
    out = run(programs, which, "cond-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(shapes), len(m.FIELDS))
    want = m.plans(shapes)
    for col, field in enumerate(m.FIELDS):
        bad = np.flatnonzero(got[:, col] != want[:, col])
        assert len(bad) == 0, (field, len(bad), shapes[bad[0]].tolist(), int(got[bad[0], col]), int(want[bad[0], col]))
    plan = {f: got[:, c] for c, f in enumerate(m.FIELDS)}
    stage, n_cus, wg, count = shapes[:, 0], shapes[:, 1], shapes[:, 2], shapes[:, 3]
    assert set(np.unique(stage)) == set(range(11))
    loop = (stage != m.WIDEN) & (stage != m.UNPACK)                   # the stages that walk their streams in launches
    k = np.array([m.K.get(int(s), 0) for s in stage])
    k = np.where(k == 0, count, k)
    assert np.array_equal(plan["sum_ns"][loop], count[loop]) and np.array_equal(plan["in_order"][loop], plan["n_chunks"][loop])
    assert (plan["max_ns"][loop] <= k[loop]).all() and (plan["n_chunks"][loop] == -(-count[loop] // k[loop])).all()
    assert (plan["s0_first"] == 0).all() and np.array_equal((plan["s0_last"] + plan["ns_last"])[loop], count[loop])
    want_cap = np.where(stage == m.TONES, 8 * n_cus, np.where(stage == m.QUALITY, 64 * n_cus, n_cus * wg))
    assert np.array_equal(plan["cap"], want_cap)
    assert (plan["min_gx"][loop] >= 1).all() and (plan["max_gx"][loop] <= plan["cap"][loop]).all()
    assert (plan["gx_first"] >= 1).all() and (plan["gx_first"] <= plan["cap"]).all()          # (widen and unpack: their one launch)
    rows = (stage == m.CONDITION) | (stage == m.HIST)
    assert np.array_equal(plan["gy_first"][rows], plan["ns_first"][rows]) and np.array_equal(plan["gy_last"][rows], plan["ns_last"][rows])
    assert (plan["gy_first"][loop & ~rows] == 1).all() and (plan["gy_last"][loop & ~rows] == 1).all() and plan["gy_first"].max() == 8
    # rows side by side never take more than the cap between them, unless every one of them is down to its one workgroup
    assert ((plan["gx_first"] * plan["gy_first"] <= plan["cap"]) | (plan["gx_first"] == 1))[rows].all()
    assert (plan["lds_bytes"] <= 128 * 1024).all() and (plan["lds_bytes"][stage != m.NOTCH] == 0).all()
    assert set(np.unique(plan["lds_bytes"][:len(sweep)])) == {0, 8, 16, 8 * 1023, 8 * 16384}
    assert set(np.unique(plan["vec4"][stage == m.CONDITION])) == {0, 1} and set(np.unique(plan["vec4"][stage == m.UNPACK])) == {0, 1}
    for row, (shape, expected) in zip(got[len(sweep):], literals):
        p = dict(zip(m.FIELDS, row.tolist()))
        for field, value in expected.items():
            assert p[field] == value, (shape, field, p[field])


# ------------------------------------------------------------------------------------------------------------ cond-chain
@pytest.mark.parametrize("which", BOTH)
def test_cond_chain(programs, tmp_path, which):
    """Conditioning::upstream_of(s) (csrc/ingest.hpp) for the 16 combinations of stages on and off x the 4 stages: the stages in front
    of s are as they were, s and the ones behind it are off, a stage that is switched off keeps its values, and the notch list,
    which is its own switch, is cleared."""
    import cond_plan_model as m

    indir(tmp_path)
    out = run(programs, which, "cond-chain", tmp_path)
    rows = np.fromfile(out / "chain.i64", dtype="<i8").reshape(16 * 4, 2 + 2 * m.CHAIN_ROW)
    assert rows[:, :2].tolist() == [[combo, s] for combo in range(16) for s in range(4)]
    for combo, s, *both in rows.tolist():
        before, after = both[:m.CHAIN_ROW], both[m.CHAIN_ROW:]
        assert [int(before[i] != 0) for i in m.CHAIN_SWITCH] == [combo >> t & 1 for t in range(4)]      # the combination it says
        assert after == m.upstream_of(before, s), (combo, s)
        first = m.CHAIN_FIELDS[s][0]
        assert after[:first] == before[:first] and not any(after[m.CHAIN_SWITCH[t]] for t in range(s, 4)), (combo, s)


# ------------------------------------------------------------------------------------------------------------ dev-mem
# Byte offsets of the sub-arrays of the two scratch buffers that hold several arrays, and each buffer's size, for n_cells = 56,
# n_rows = 3 (x 7 bins = 21 grid cells), max_units = 5; from the pointer arithmetic these buffers were carved with by hand:
#   acquisition's bookkeeping: gyp_cell prev_out[n_cells] (32 bytes each), then int32 reuse[n_cells], order[n_cells], cand[n_cells],
#     n_active, n_cand, n_pend; n_cells * (32 + 3 * 4) + 64 bytes
#   the refine list: int32 n_cand[4], pend_rows[n_rows], pend_first[n_rows], cand[n_cells]; (n_cells + 2 n_rows + 4) * 4 bytes
#   the shared-forward unit lists: int32 unit_cell[max_units], sh_cell[n_cells], sh_unit[n_cells], counts[4]; (max_units + 2 n_cells + 4) * 4 bytes
CARVE_LITERALS = [0, 1792, 2016, 2240, 2464, 2468, 2472, 2528,
                  0, 16, 28, 40, 124,
                  0, 20, 244, 468, 484]
INHERITED_SWITCHES = {"no_pipe", "no_shared_fwd", "no_acq_shared_fwd", "symbol_tau", "cells_cu_reserve", "track_chunk_ms", "no_spec", "track_finish_all"}


@pytest.mark.parametrize("which", BOTH)
def test_dev_mem(programs, tmp_path, which):
    """The owners of dev_mem.hpp where every allocation fails (no device), the scratch layouts against the offsets above, and every row
    of the table of debug switches on a context on the stack (the driver checks ranges, set / get and refusals itself)."""
    d = indir(tmp_path)
    i64([56, 3, 5]).tofile(d / "layouts.i64")
    out = run(programs, which, "dev-mem", tmp_path)
    assert np.fromfile(out / "carve.i64", dtype="<i8").tolist() == CARVE_LITERALS
    rows = [line.split() for line in (out / "switches.txt").read_text().splitlines()]
    names = [r[0] for r in rows]
    assert len(rows) == 24 and len(set(names)) == len(names)
    for name, lo, hi, integral, inherited, default in rows:
        assert float(lo) <= float(default) <= float(hi), name
    assert {r[0] for r in rows if r[4] == "1"} == INHERITED_SWITCHES
    by_name = {r[0]: r for r in rows}
    assert [float(x) for x in by_name["grid_fused_waves"][1:3]] == [8.0, 12.0] and float(by_name["grid_fused_waves"][5]) == 12.0
    assert [float(x) for x in by_name["track_chunk_ms"][1:3]] == [0.0, 1e6] and float(by_name["track_chunk_ms"][5]) == 250.0
    assert by_name["symbol_tau"][3] == "0" and by_name["dll_prov_bias"][3] == "0" and sum(r[3] == "0" for r in rows) == 2
    assert [float(x) for x in by_name["hybrid_scratch_mb"][1:3]] == [16.0, 65536.0] and float(by_name["hybrid_scratch_mb"][5]) == 1024.0
    for name in ("notch_no_lds", "track_finish_all"):
        assert [float(x) for x in by_name[name][1:3]] == [0.0, 1.0] and by_name[name][3] == "1" and float(by_name[name][5]) == 0.0


# ------------------------------------------------------------------------------------------------------------ hybrid-plan
def f64(rows) -> np.ndarray:
    return np.array(rows, dtype="<f8")


def search_rows():
    """(n, n_streams, n_sats, T, blocks, flags, center, spread, step, scratch_mb) of the weak_search_plan rows: per T the coarse level at
    1, 4096 and 4097 bins (bins every 500 / T Hz over [-spread, spread)) crossed with the fine level at 0, 1, 4095 and 4097 bins (2 J + 1
    with J steps within 250 / T Hz); states x bins on both sides of 2^31 - 1; 32 and 33 satellites; and a row per refusal in front."""
    rows = []
    for T in (1, 2, 20):
        bin_hz, half_hz = 500.0 / T, 250.0 / T
        for spread in (bin_hz / 2, 2048 * bin_hz, 2048.5 * bin_hz):
            for step in (0.0, 2 * half_hz, half_hz / 2047.5, half_hz / 2048):
                rows.append((2046, 2, 3, T, 4, 3, 100.0, spread, step, 16))
        # 4096 coarse bins: 524287 x 4096 = 2^31 - 4096, 524288 x 4096 = 2^31
        rows += [(2046, ns, sats, T, 1, 0, 0.0, 2048 * bin_hz, 0.0, 1024) for ns, sats in ((524287, 1), (524288, 1), (16383, 32), (16384, 32), (16384, 33))]
        rows += [(2046, 1, sats, T, 2, 1, 0.0, 7000.0, 10.0, 1024) for sats in (32, 33)]
    nan, inf = float("nan"), float("inf")
    rows += [(2046, 1, 1, T, M, flags, 0.0, 500.0, 0.0, 1024) for T, M, flags in ((0, 1, 0), (21, 1, 0), (1, 0, 0), (16, 4096, 0), (1, 2, 4), (1, 1, 1), (0, 0, 4))]
    rows += [(2046, 1, 1, 1, 1, 0, c, s, f, 1024) for c, s, f in ((nan, 500.0, 0.0), (inf, 500.0, 0.0), (0.0, nan, 0.0), (0.0, inf, 0.0), (0.0, 500.0, nan),
                                                                  (0.0, 500.0, -inf), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), (1e300, 1.0, 0.0), (0.0, 500.0, -1.0))]
    rows += [(2046, 1, 33, 1, 1, 0, nan, 500.0, 0.0, 1024), (2046, 1, 1, 1, 1, 0, 0.0, 0.0, 250.0 / 2048, 1024), (49104, 4, 8, 20, 3, 3, -3000.0, 7000.0, 1.0, 16)]
    return rows


@pytest.mark.parametrize("which", BOTH)
def test_hybrid_plan(programs, tmp_path, which):
    """hybrid_plan, hybrid_coarse_bins / hybrid_coarse_bin / hybrid_fine_half, hybrid_shift, hybrid_z and weak_search_plan
    (csrc/hybrid_plan.hpp) against tests/hybrid_model.py, every comparison exact: the model restates the same integer and float64
    operations.  The scenario also checks on a context on the stack that gyp_acquire_weak_dev refuses with the plan's texts before
    anything is planned into the context."""
    import hybrid_model as hm

    d = indir(tmp_path)
    plans = [(n, cells, mb, flags, T, M) for n in (1023, 2046, 49104) for cells in (0, 1, 2, 511, 512, 513, 65535, 65536, 2 ** 31 - 1, 2 ** 31)
             for mb in (16, 1024, 65536) for flags in (0, 1, 2, 3, 4) for T, M in ((1, 1), (20, 1), (2, 4), (21, 1), (1, 65536))]
    i64(plans).tofile(d / "plans.i64")
    bins = []
    for T in (1, 2, 10, 20):
        edge = 250.0 / T
        for spread in (np.nextafter(edge, 0.0), edge, 7000.0, 1e9):
            for step in (0.0, -1.0, float("nan"), 1e-9, 10.0, edge, np.nextafter(edge, np.inf)):
                bins.append((T, 0.0, spread, step))
                bins.append((T, -4321.5, spread, step))
    f64(bins).tofile(d / "bins.f64")
    shifts = [(n, T, b, sign * f, flags) for n, T, b in ((1023, 1, 1), (2046, 10, 21), (2046, 20, 3276), (8184, 4, 1000), (49104, 1, 65535), (2046, 1, 0))
              for f in (0.0, 1.0, 4487.0, 7000.0, 200000.0, 770000.0, np.nextafter(770000.0, 0.0), 1e300, float("inf"), float("nan")) for sign in (1.0, -1.0)
              for flags in (0, 1, 2, 3)]
    from fractions import Fraction
    for n, T, b in ((1023, 1, 1), (2046, 1, 1), (1023, 4, 4), (2046, 4, 2), (1023, 10, 1), (8184, 1, 2), (2046, 10, 1)):      # exact halves (test_hybrid_host.py)
        for k in (0, 1, 7, 3000):
            exact = Fraction((2 * k + 1) * 1575420000, 2 * b * T * n)
            if Fraction(float(exact)) == exact:
                shifts += [(n, T, b, sign * f, 2) for f in (float(exact), np.nextafter(float(exact), 0.0), np.nextafter(float(exact), np.inf)) for sign in (1.0, -1.0)]
    halves = len(shifts) - 6 * 10 * 2 * 4
    assert halves >= 6 * 20
    f64(shifts).tofile(d / "shifts.f64")
    zs = [(5.0, 0, 0.0, 0.0), (5.0, -1, 1.0, 1.0), (5.0, 100, 200.0, 400.0), (5.0, 3, 0.3, 0.03 * (1 - 1e-15)), (4.0, 4, 4.0, 8.0), (1.0, 10, 1.0, 1.0),
          (0.0, 10, 1.0, 1.0), (7.5, 2045, 3.25e3, 9.5e3), (float("inf"), 10, 1.0, 2.0), (1.0, 10, float("nan"), 1.0), (1.0, 10, 1.0, float("nan")),
          (3.0, 2 ** 31 - 1, 1e9, 1e10), (2.0, 7, 2.0, 2.0)]
    f64(zs).tofile(d / "zs.f64")
    searches = search_rows()
    f64(searches).tofile(d / "searches.f64")

    out = run(programs, which, "hybrid-plan", tmp_path)
    got = np.fromfile(out / "plans.i64", dtype="<i8").reshape(len(plans), len(hm.PLAN_FIELDS)).tolist()
    for (n, cells, mb, flags, T, M), row in zip(plans, got):
        assert tuple(row) == hm.plan(n, cells, T, M, flags, mb), (n, cells, mb, flags, T, M)
    fits = {p[:6]: r[0] for p, r in zip(plans, got)}
    assert fits[2046, 1, 16, 3, 2, 4] == 1 and fits[2046, 0, 16, 0, 1, 1] == 0 and fits[2046, 2 ** 31, 16, 0, 1, 1] == 0 and fits[2046, 1, 16, 4, 1, 1] == 0
    by_shape = {p: dict(zip(hm.PLAN_FIELDS, r)) for p, r in zip(plans, got)}
    assert by_shape[2046, 513, 16, 3, 2, 4]["chunk_cells"] == 512 and by_shape[2046, 513, 16, 3, 2, 4]["n_chunks"] == 2      # 16 MiB / 32736 bytes
    assert by_shape[1023, 2 ** 31 - 1, 65536, 0, 1, 1]["chunk_cells"] == 65535 and by_shape[49104, 65536, 16, 1, 2, 4]["chunk_cells"] == 21
    got = np.fromfile(out / "bins.i64", dtype="<i8").reshape(len(bins), 4).tolist()
    for (T, center, spread, step), (n_coarse, half, first, last) in zip(bins, got):
        assert n_coarse == hm.n_coarse(center, spread, T) and half == hm.fine_half(step, T), (T, center, spread, step)
        assert first == f64([center - spread]).view("<i8")[0] and last == f64([center - spread + float(max(n_coarse - 1, 0)) * (500.0 / T)]).view("<i8")[0]
        if n_coarse < 1000:      # the lists the model's search walks, where they are short
            assert n_coarse == len(hm.coarse_bins(center, spread, T))
        if 0 <= half < 1000:
            assert 2 * half + 1 == len(hm.fine_bins(0.0, step, T))
        elif half < 0:
            assert hm.fine_bins(0.0, step, T) == []
    seen = {(r[0], r[1]) for r in got}
    assert {n for n, _ in seen} >= {1, 28, 560, 1_000_000} and {h for _, h in seen} >= {-1, 0, 1, 500_000}      # both caps, both edges
    got = np.fromfile(out / "shifts.i64", dtype="<i8").tolist()
    assert got == [hm.shift(n, T, b, f, flags) if np.isfinite(f) and abs(float(b * T * n) * f / hm.L1_HZ) < 2147483000.0 else 0 for n, T, b, f, flags in shifts]
    assert min(got) < -1000 and max(got) > 1000
    got = np.fromfile(out / "zs.f64", dtype="<f8").reshape(len(zs), 2)
    want = f64([(hm.z_of(float(np.float32(peak)), n_off, s, ss), 1.0 if ss > s else 0.0) for peak, n_off, s, ss in zs])
    assert got.tobytes() == want.tobytes() and np.isnan(got[:4, 0]).all() and got[4, 0] == 3.0
    why = (out / "searches.txt").read_text().splitlines()
    got = np.fromfile(out / "searches.i64", dtype="<i8").reshape(len(searches), len(hm.SEARCH_FIELDS)).tolist()
    for shape, text, row in zip(searches, why, got):
        n, ns, sats, T, M, flags, center, spread, step, mb = shape
        want_why, want_row = hm.weak_search_plan(n, ns, sats, T, M, flags, center, spread, step, mb)
        assert text == (want_why or "ok") and tuple(row) == want_row, shape
    assert set(why) == {"ok", "coherent_ms must be 1..20", "n_blocks must be at least 1", "n_blocks * coherent_ms must be at most 65535", "unknown flag bits",
                        "GYP_HYB_ALTERNATE needs at least 2 blocks", "at most 32 satellites per call",
                        "center, spread and fine step must be finite and the spread positive", "a level must have between 1 and 4096 Doppler bins",
                        "more than 2^31 - 1 cells"}
    ok = [dict(zip(hm.SEARCH_FIELDS, r)) for r, t in zip(got, why) if t == "ok"]
    assert {p["n_coarse"] for p in ok} >= {1, 4096} and {p["n_fine"] for p in ok} >= {0, 1, 4095} and max(p["records"] for p in ok) == 2 ** 31 - 4096
    assert all(p["run_fits"] == 1 and p["level_cells"] == p["coarse_cells"] + p["fine_cells"] + p["n_states"] for p in ok)


# ------------------------------------------------------------------------------------------------------------ weak-plan
@pytest.mark.parametrize("which", BOTH)
def test_weak_plan(programs, tmp_path, which):
    """The host copy of the weak bank's arithmetic (csrc/weak_plan.hpp) against tests/weak_track_model.py, every comparison exact:
    the refusals, a channel's start-up, the code rate and the NCO advances, the bit-edge energies, and weak_fold_ms + weak_close_period
    over 26 periods of fixed prompts -- the 25-entry mu ring wraps once and lose_mu trips."""
    import weak_track_model as wm

    d = indir(tmp_path)
    lib = _lib.load()
    default = np.zeros(1, dtype=_lib.WEAK_PARAMS)
    lib.gyp_weak_params_default(_lib.ptr(default))
    up, down = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    edges = [{}, dict(period_ms=19), dict(period_ms=21), dict(sync_ms=39), dict(sync_ms=40), dict(sync_ms=2000), dict(sync_ms=2001), dict(spacing=0),
             dict(spacing=1), dict(spacing=wm.ONE), dict(spacing=wm.ONE + 1), dict(pll_bw_hz=0.0), dict(pll_bw_hz=up(0.0)), dict(pll_bw_hz=50.0),
             dict(pll_bw_hz=up(50.0)), dict(pll_bw_hz=float("nan")), dict(dll_bw_hz=0.0), dict(dll_bw_hz=up(0.0)), dict(dll_bw_hz=10.0),
             dict(dll_bw_hz=up(10.0)), dict(dll_bw_hz=float("nan")), dict(lose_mu=down(0.0)), dict(lose_mu=0.0), dict(lose_mu=20.0), dict(lose_mu=up(20.0)),
             dict(lose_mu=float("nan")), dict(period_ms=10, sync_ms=39), dict(sync_ms=39, spacing=0), dict(spacing=0, pll_bw_hz=0.0),
             dict(pll_bw_hz=0.0, dll_bw_hz=0.0), dict(dll_bw_hz=0.0, lose_mu=21.0)]
    params = np.repeat(default, len(edges))
    for rec, change in zip(params, edges):
        for k, v in change.items():
            rec[k] = v
    params.tofile(d / "params.bin")
    init_rows = [(0, 1, 0.0, 0.0), (-1, 1, 0.0, 0.0), (0, 0, 0.0, 0.0), (0, 32, 0.0, 0.0), (0, 33, 0.0, 0.0), (0, 1, float("nan"), 0.0), (0, 1, float("inf"), 0.0),
                 (0, 1, 0.0, float("nan")), (0, 1, 0.0, -float("inf")), (-1, 0, 0.0, 0.0), (0, 0, float("nan"), 0.0), (0, 1, float("nan"), float("nan")),
                 (2 ** 31 - 1, 1, -1e300, 1e300)]
    inits = np.zeros(len(init_rows), dtype=_lib.CHAN_INIT)
    for rec, (stream, sat, dop, phase) in zip(inits, init_rows):
        rec["stream"], rec["sat_id"], rec["doppler_hz"], rec["carrier_phase"] = stream, sat, dop, phase
    inits.tofile(d / "inits.bin")
    fresh = [(n, cursor, stream, sat, dop, phase, code) for n in (1023, 2046, 49104) for code in (0, 1, n - 1)
             for cursor, stream, sat, dop, phase in ((0, 0, 1, 1234.5, 0.0), (100, 3, 32, -4999.25, -1e-300), (2 ** 40, 1, 7, 0.0, 2 * np.pi), (7, 2, 9, 1e-3, -2 * np.pi),
                                                    (19, 0, 5, 250.0, 1.0), (20, 0, 5, -250.0, -1.0))]
    i64([(n, cursor) for n, cursor, *_ in fresh]).tofile(d / "fresh.i64")
    fresh_inits = np.zeros(len(fresh), dtype=_lib.CHAN_INIT)
    for rec, (_, _, stream, sat, dop, phase, code) in zip(fresh_inits, fresh):
        rec["stream"], rec["sat_id"], rec["doppler_hz"], rec["carrier_phase"], rec["code_phase"] = stream, sat, dop, phase, code
    fresh_inits.tofile(d / "inits_fresh.bin")
    rates = [(f, n) for n in (1023, 2046, 49104) for f in (0.0, 1.0, -1.0, 4999.75, -4999.75, 1e5, -1e5, 1575.42e6, -1575.42e6)]
    f64(rates).tofile(d / "rates.f64")
    advances = [(u0, f, fs, c0, samples, r) for u0, f in ((0.0, 0.0), (0.25, 1234.5), (0.999999, -4999.75), (0.5, -1e5)) for fs in (1.023e6, 2.046e6, 49.104e6)
                for c0, samples, r in ((0, 2046, wm.code_rate(0.0, 2046)), (-1, 1023, wm.ONE), (-wm.CODE_MOD, 20 * 49104, wm.code_rate(-4999.75, 49104)),
                                       (wm.CODE_MOD, 0, 5), (3 * wm.CODE_MOD + 7, -2046, wm.code_rate(1e5, 2046)), (-5 * wm.CODE_MOD - 7, -1, 1))]
    f64([a[:3] for a in advances]).tofile(d / "advances.f64")
    i64([a[3:] for a in advances]).tofile(d / "advances.i64")
    rng = np.random.default_rng(20261021)
    firsts = [0, 7, 19, 20, 33, 2 ** 40 + 13]
    prompts = {}
    for edge in (0, 7, 19):      # 40 ms of prompts whose sign flips at the milliseconds m with m % 20 == edge, for first_ms 0: +- 1 and noise
        m = np.arange(40)
        sign = np.where(((m - edge) // 20) % 2 == 0, 1.0, -1.0)
        prompts[edge] = (sign * (1.0 + 0.5j) + 0.3 * (rng.standard_normal(40) + 1j * rng.standard_normal(40))).astype(np.complex64)
    loop_ms = (rng.standard_normal((26 * 20, 6)) * 40.0).astype(np.float32)
    loop_ms[:, 2] += 300.0                                      # a prompt on the I axis ...
    loop_ms[10 * 20:, 2:4] = (rng.standard_normal((16 * 20, 2)) * 300.0).astype(np.float32)      # ... that is lost from period 10 on: mu falls below lose_mu
    loop_ms.tofile(d / "loop.f32")
    loop_f, loop_i = (1234.5, 0.625, 2.046e6, 8.0, 1.0, 9.0), (wm.init_c0(777, 2046), 2046, 113)
    f64(loop_f).tofile(d / "loop.f64")
    i64(loop_i).tofile(d / "loop.i64")

    np.concatenate(list(prompts.values())).view(np.float32).tofile(d / "sync.f32")
    i64(firsts).tofile(d / "sync.i64")

    out = run(programs, which, "weak-plan", tmp_path)
    got_sync = dict(zip(prompts, np.fromfile(out / "sync.f64", dtype="<f8").reshape(len(prompts), len(firsts), 21)))
    for edge, p in prompts.items():
        for row, first in zip(got_sync[edge], firsts):
            en, pick = wm.bit_sync(p, first)
            assert row[:20].tobytes() == en.tobytes() and int(row[20]) == pick, (edge, first)
        assert int(got_sync[edge][0, 20]) == edge and int(got_sync[edge][1, 20]) == (edge + 7) % 20      # first_ms 0 finds the edge; first_ms 7 sees it 7 later
    lines = (out / "refusals.txt").read_text().splitlines()
    want = [wm.params_refusal(int(r["period_ms"]), int(r["sync_ms"]), int(r["spacing"]), float(r["pll_bw_hz"]), float(r["dll_bw_hz"]), float(r["lose_mu"])) for r in params]
    want += [wm.init_refusal(*row) for row in init_rows]
    assert lines == [w or "ok" for w in want]
    assert lines[:len(edges)].count("ok") == 11 and lines[len(edges):].count("ok") == 3 and len(set(lines)) == 11      # every refusal of both functions
    assert (out / "default.bin").read_bytes() == default.tobytes()
    chans = np.fromfile(out / "fresh.bin", dtype=wm.CHAN)
    assert len(chans) == len(fresh)
    for got, (n, cursor, stream, sat, dop, phase, code) in zip(chans, fresh):
        assert got.tobytes() == wm.fresh_chan(stream, sat, dop, phase, code, n, cursor).tobytes(), (n, cursor, phase, code)
    assert (chans["u0"] >= 0.0).all() and (chans["u0"] < 1.0).all() and (chans["c0"] >= 0).all() and (chans["c0"] < wm.CODE_MOD).all()
    assert np.fromfile(out / "rates.i64", dtype="<i8").tolist() == [wm.code_rate(f, int(n)) for f, n in rates]
    adv_u, adv_c = np.fromfile(out / "advanced.f64", dtype="<f8"), np.fromfile(out / "advanced.i64", dtype="<i8").reshape(-1, 2)
    for (u0, f, fs, c0, samples, r), got_u, (got_mod, got_c) in zip(advances, adv_u.tolist(), adv_c.tolist()):
        want_u, want_c = wm.advance(u0, c0 % wm.CODE_MOD, f, fs, samples, r)
        assert (got_u, got_mod, got_c) == (want_u, c0 % wm.CODE_MOD, want_c), (u0, f, fs, c0, samples, r)
    # the loop: 26 periods folded and closed
    s = np.zeros(1, dtype=wm.CHAN)[0]
    s["phase"], s["f"], s["f_int"], s["u0"], s["c0"] = wm.TRACK, loop_f[0], loop_f[0], loop_f[1], loop_i[0]
    prm = wm.Params(pll_bw_hz=loop_f[3], dll_bw_hz=loop_f[4], lose_mu=loop_f[5])
    periods = np.fromfile(out / "periods.bin", dtype=_lib.WEAK_PERIOD_REC)
    assert len(periods) == 26
    for k, got in enumerate(periods):
        s["period_first"] = loop_i[2] + 20 * k
        for row in loop_ms[20 * k:20 * k + 20]:
            wm.fold_ms(s, complex(row[0], row[1]), complex(row[2], row[3]), complex(row[4], row[5]))
            s["pos"] += 1
        want = wm.close_period(s, prm, loop_f[2], loop_i[1])
        rec = np.zeros(1, dtype=_lib.WEAK_PERIOD_REC)
        for name in wm.PERIOD_FIELDS:
            rec[name] = want[name]
        assert got.tobytes() == rec.tobytes(), (k, got, rec)
    assert (out / "chan.bin").read_bytes() == s.tobytes()
    assert periods["mu_mean"][:24].tolist() == [0.0] * 24 and periods["mu_mean"][24] > 0.0 and int(s["n_periods"]) == 26 and int(s["status"]) == 2
    assert 1 in periods["status"][24:].tolist() and (periods["mu"][:10] > 10.0).all() and periods["bit"][:10].tolist() == [1] * 10
