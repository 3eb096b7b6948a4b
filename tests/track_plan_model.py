"""Python restatement of what a gyp_track_block_dev call runs (gypsum_amd/csrc/track_plan.hpp): the flow, the sub-blocks and rounds of a
speculative block, the throughput kernel's launch length and launches, the exact-sums kernel, the confidence threshold.  Written from the
host code as it stood before the header existed (the `light` predicate, the speculative tracker's sub-block count, layout and rounds, the
throughput path's chunks and exact-sums choice, the threshold's correction by rate).  Every argument of track_plans may be an array (they
broadcast).  tests/test_host_sanitizers.py::test_track_plan compares the two over a sweep; tests/test_gpu_track_plan.py asks it what a
call must have run.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SUB_BLOCKS = 32          # SubLayout holds 32 sub-blocks
MAX_SUB = 20                 # ... and a layout of 500-ms sub-blocks at most 20 + 2
EXACT_GROUP_MAX_CHAN = 16384
ROUND_PROTOCOL_MAX_CHAN = 24
FIELDS = ("flow", "rounds", "chunk_ms", "launches", "exact_path", "spec_kappa_bits", "n", "longest") + tuple(f"start{i}" for i in range(MAX_SUB_BLOCKS + 1))


def layout(n_ms: int, sub_ms: int):
    """(starts, longest): the first milliseconds of a speculative block's sub-blocks (target length sub_ms) and the longest one's length."""
    cap = MAX_SUB if sub_ms == 500 else MAX_SUB_BLOCKS - 2
    n_sub = min(cap, max(4, n_ms // sub_ms)) if n_ms >= 2048 else (4 if n_ms >= 256 else 1)
    length = -(-n_ms // n_sub)
    if n_sub > 1 and length >= 160:      # three shrinking pieces in place of the last sub-block
        t1, t2, t3 = -(-56 * length // 100), -(-34 * length // 100), max(32, length // 5)
        piece = -(-(n_ms - (t1 + t2 + t3)) // (n_sub - 1))
        pieces = [piece] * (n_sub - 1) + [t1, t2, n_ms]      # (the last one: whatever is left)
    else:
        pieces = [length] * n_sub
    starts, at, longest = [], 0, 0
    for p in pieces:
        if p <= 0 or at >= n_ms or len(starts) >= MAX_SUB_BLOCKS:
            continue
        p = min(p, n_ms - at)
        starts.append(at)
        longest = max(longest, p)
        at += p
    return starts, longest


def track_plans(k, n, n_cus, n_chan, n_ms, keep_profiles=0, no_pipe=0, no_spec=0, spec_redo=1, spec_sub_ms=0, track_chunk_ms=250,
                no_exact_shared=0, kappa=20.0) -> np.ndarray:
    """int64 [rows, len(FIELDS)] over the broadcast of the arguments (spec_kappa as the bits of the float32)."""
    kappa = np.asarray(kappa, dtype=np.float64)
    cols = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in (k, n, n_cus, n_chan, n_ms, keep_profiles, no_pipe, no_spec, spec_redo,
                                                                         spec_sub_ms, track_chunk_ms, no_exact_shared)], kappa)
    k, n, n_cus, n_chan, n_ms, keep, no_pipe, no_spec, redo, sub_ms, chunk_ms, no_shared = [c.ravel() for c in cols[:12]]
    kappa = cols[12].ravel()
    out = np.zeros((k.size, len(FIELDS)), dtype=np.int64)
    light = np.isin(k, (2, 8, 16)) & (n_chan <= n_cus) & (no_pipe == 0)
    plain = (keep != 0) | ~light | (no_spec != 0)                              # the throughput kernel
    sub_ms = np.where(sub_ms >= 100, sub_ms, np.where(k == 2, 167, 500))       # "spec_sub_ms": from 100 on the value, below (0, 1..99) by rate
    for key in np.unique(np.stack([n_ms, sub_ms], axis=1)[~plain], axis=0):
        starts, longest = layout(int(key[0]), int(key[1]))
        rows = ~plain & (n_ms == key[0]) & (sub_ms == key[1])
        out[rows, 6], out[rows, 7] = len(starts), longest
        out[rows, 8:] = starts + [int(key[0])] * (MAX_SUB_BLOCKS + 1 - len(starts))
    n_sub = out[:, 6]
    flow = np.where(plain, 1, np.where((n_sub == 1) | (redo == 0) | (n_chan > ROUND_PROTOCOL_MAX_CHAN), 2, 3))
    out[:, 0] = flow
    out[:, 1] = np.select([flow == 3, flow == 2], [n_sub + 2 + np.where(n_sub >= 8, 6, 2), 1], 0)      # (flow 2: the round tables keep one row)
    out[:, 2] = np.where(plain & (chunk_ms > 0), chunk_ms, n_ms)               # the re-run behind a speculative block: one launch
    out[:, 3] = -(-n_ms // out[:, 2])
    shared = plain & (k == 8) & (no_shared == 0) & (n_chan <= EXACT_GROUP_MAX_CHAN)
    out[:, 4] = np.where(shared, 2, np.where(k <= 8, 1, 3))
    log_rate = np.zeros(k.size)
    for v in np.unique(n):
        log_rate[n == v] = math.log(int(v) / 8184.0)
    corrected = np.maximum(0.0, kappa + np.where(kappa > 0.0, log_rate + np.where(k == 2, -5.0, 0.0), 0.0))
    out[:, 5] = np.where(plain, kappa, corrected).astype(np.float32).view(np.uint32)
    return out


def track_plan(*args, **kwargs) -> dict:
    """The same for one shape, as plain ints, with the sub-block starts [0, ..., n_ms] under "starts"."""
    row = track_plans(*args, **kwargs)[0].tolist()
    plan = dict(zip(FIELDS[:8], row[:8]))
    plan["starts"] = row[8:8 + plan["n"] + 1] if plan["n"] else []
    return plan
