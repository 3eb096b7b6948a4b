"""Python restatement of what the conditioning stages launch (gypsum_amd/csrc/cond_plan.hpp): the persistent grid's cap, the three
grid formulas, the cut of n streams into launches of at most K, the 16-byte-access decisions and the notch's LDS.  Written from the
launch functions as they stood before the header existed (stats_launch, condition_launch, tones_launch, notch_launch, quality_launch,
blank_launch, hist_launch, widen_launch, unpack_launch).  tests/test_host_sanitizers.py::test_cond_plan compares the two over a sweep.

A shape is a row of int64: (stage, n_cus, wg_per_cu, n, a, b, stride, in_addr, out_addr, flag) with
    STATS      n streams, a = n_ms
    CONDITION  n streams, a = n_samples, stride, in_addr, out_addr
    NOTCH      n streams, a = n_ms, b = samples per millisecond, flag = notch_no_lds
    BLANK      n streams, a = n_ms
    HIST       n streams, a = n_samples
    TONES      n streams, a = n_blocks, b = n_freq
    QUALITY    n channels, a = n_ms, b = window_ms
    WIDEN      a = n_words
    UNPACK     n streams, a = n_samples, b = bits per component, stride, out_addr
    EXCISE     n streams, a = n_ms
    SPECTRUM   n streams, a = n_ms (the excisor's histogram: every stream in one launch)
A plan is a row of FIELDS: the first and the last launch of the call, and over all launches the sum and the largest of their stream
counts, how many start where the one before ended, and the smallest and largest grid.x.
"""
from __future__ import annotations

import numpy as np

STATS, CONDITION, NOTCH, BLANK, HIST, TONES, QUALITY, WIDEN, UNPACK, EXCISE, SPECTRUM = range(11)
# streams (channels) per launch: kLevelStreams, kNotchStreams, kBlankStreams (both blanker kernels), kQualityChans, kExciseStreams
K = {CONDITION: 8, NOTCH: 8, BLANK: 8, HIST: 8, QUALITY: 1024, EXCISE: 8}
NOTCH_LDS_SAMPLES = 16384
SHAPE_COLUMNS = ("stage", "n_cus", "wg_per_cu", "n", "a", "b", "stride", "in_addr", "out_addr", "flag")
FIELDS = ("n_chunks", "vec4", "lds_bytes", "per_stream", "cap",
          "s0_first", "ns_first", "gx_first", "gy_first", "items_first", "s0_last", "ns_last", "gx_last", "gy_last", "items_last",
          "sum_ns", "max_ns", "in_order", "min_gx", "max_gx")


def ceil_div(a, b):
    return -(-a // b)


def grid_per_item(items, cap):
    return np.minimum(items, cap)


def grid_per_row(v, cap, ns):
    return np.maximum(1, np.minimum(ceil_div(v, 256), np.maximum(1, cap // ns)))


def grid_widen(n_words, cap):
    return np.minimum(ceil_div(n_words // 16, 256) + 1, cap)


def plans(shapes: np.ndarray) -> np.ndarray:
    """int64 [rows, len(FIELDS)] for int64 shapes [rows, len(SHAPE_COLUMNS)]."""
    stage, n_cus, wg, n, a, b, stride, in_addr, out_addr, flag = np.asarray(shapes, dtype=np.int64).T
    is_ = {s: stage == s for s in range(11)}
    cap = np.where(is_[TONES], n_cus * 8, np.where(is_[QUALITY], n_cus * 64, n_cus * wg))
    k = n.copy()                                                  # statistics, tones and the spectrum histogram: every stream in one launch
    for s, per_launch in K.items():
        k[is_[s]] = per_launch
    per_row = is_[CONDITION] | is_[HIST]
    # 16-byte accesses: aligned bases, and rows that stay aligned (one stream, or an even stride)
    vec4 = np.where(is_[CONDITION], ((in_addr | out_addr) % 16 == 0) & ((n == 1) | (stride % 2 == 0)),
                    np.where(is_[UNPACK], (out_addr % 16 == 0) & (stride % 2 == 0), False)).astype(np.int64)
    lds = np.where(is_[NOTCH] & (b <= NOTCH_LDS_SAMPLES) & (flag == 0), 8 * b, 0)
    with np.errstate(divide="ignore"):
        windows = ceil_div(a, np.where(is_[QUALITY], b, 1))
    per_stream = np.select([is_[STATS] | is_[NOTCH] | is_[BLANK] | is_[EXCISE] | is_[SPECTRUM], is_[CONDITION], is_[HIST], is_[TONES], is_[QUALITY]],
                           [a, np.where(vec4 == 1, (a + 1) // 2, a), a // 2, a * b, windows], 0)
    n_chunks = ceil_div(n, np.maximum(k, 1))

    def chunk(i):
        s0 = i * k
        ns = np.minimum(k, n - s0)
        items = np.where(per_row, per_stream, ns * per_stream)
        gx = np.where(per_row, grid_per_row(per_stream, cap, np.maximum(ns, 1)),
                      grid_per_item(np.where(is_[QUALITY], ceil_div(items, 4), items), cap))
        return s0, ns, gx, np.where(per_row, ns, 1), items

    first, last = chunk(np.zeros_like(n)), chunk(n_chunks - 1)
    out = np.stack([n_chunks, vec4, lds, per_stream, cap, *first, *last, n, np.minimum(n, k), n_chunks,
                    np.minimum(first[2], last[2]), np.maximum(first[2], last[2])], axis=1)
    # the two single launches outside the stream loop
    w = is_[WIDEN]
    out[w] = 0
    out[w, FIELDS.index("n_chunks")] = 1
    out[w, FIELDS.index("cap")] = cap[w]
    out[w, FIELDS.index("gx_first")] = grid_widen(a[w], cap[w])
    u = is_[UNPACK]
    items = ceil_div(a[u], 64 // np.where(u, b, 1)[u]) * n[u]
    out[u] = 0
    out[u, FIELDS.index("n_chunks")] = 1
    out[u, FIELDS.index("vec4")] = vec4[u]
    out[u, FIELDS.index("cap")] = cap[u]
    out[u, FIELDS.index("gx_first")] = np.maximum(1, np.minimum(ceil_div(items, 256), cap[u]))
    out[u, FIELDS.index("items_first")] = items
    return out


# ---------------------------------------------------------------------------------------------------- the chain
# A conditioning as a row of integers (floats as their bits), stage by stage in the chain's order: [first, end) of each stage's
# fields, and where its switch is (the notches' is their count).
CHAIN_FIELDS = ((0, 5), (5, 10), (10, 20), (20, 25))     # blanker, excisor, notches, level
CHAIN_SWITCH = (0, 5, 10, 20)
CHAIN_ROW = 25
NOTCHES = 2


def upstream_of(row, stage: int):
    """The conditioning a measurement of `stage` sees: the stages in front of it unchanged, it and the ones behind it off.  What is
    switched off keeps its values, except the notches, whose list is their switch: it is cleared."""
    out = list(row)
    for s in range(stage, len(CHAIN_FIELDS)):
        first, end = CHAIN_FIELDS[s]
        out[CHAIN_SWITCH[s]] = 0
        if s == NOTCHES:
            out[first:end] = [0] * (end - first)
    return out
