"""Recordings of 1-, 2- or 4-bit words packed into bytes (include/gypsum_hip.h, "packed recordings").

A `Packing` says how the words of such a file are laid out and what each code means; the engine unpacks them on the device
(`IqFileIngest(packing=...)`, `AntennaSampleProviderResampled(packing=...)`, `GypsumEngine.unpack_iq_dev` /
`resample_packed_dev`).  There is no CPU unpacking in the product: `pack` and `quantize` exist to write recordings.

Word w of the file occupies bits [w * bits, (w + 1) * bits) of the byte stream; within a byte the earliest word sits in the most
significant bits ("msb", GYP_PACK_MSB_FIRST) or in the least ("lsb").  Word values are levels[code] * scale.  Presets, for a
code c of b bits:

    sign_magnitude(b)   s = c >> (b - 1), m = c & (2^(b-1) - 1):  (1 - 2 s) (2 m + 1)     2 bits: +1, +3, -1, -3;  1 bit: +1, -1
    twos_complement(b)  c - 2^b if c >= 2^(b-1), else c                                     2 bits: 0, 1, -2, -1;   1 bit: 0, -1
    offset_binary(b)    2 c - (2^b - 1)                                                      2 bits: -3, -1, +1, +3;  1 bit: -1, +1

Every preset level is an integer of magnitude <= 15, so it is exact in int8: a packed file and the int8 file of its levels give
bit-identical samples.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _lib

ORDERS = {"msb": _lib.GYP_PACK_MSB_FIRST, "lsb": _lib.GYP_PACK_LSB_FIRST}


@dataclass(frozen=True)
class Packing:
    bits: int                      # 1, 2 or 4
    levels: tuple                  # 2^bits floats: the value of each code before scale
    real: bool = False             # False: words alternate I, Q; True: one real word per sample (an IF recording)
    order: str = "msb"             # "msb" or "lsb": where a byte's earliest word sits

    def __post_init__(self) -> None:
        if self.bits not in (1, 2, 4):
            raise ValueError(f"bits must be 1, 2 or 4, not {self.bits}")
        if self.order not in ORDERS:
            raise ValueError(f"order must be 'msb' or 'lsb', not {self.order!r}")
        lv = tuple(float(x) for x in self.levels)
        if len(lv) != 1 << self.bits:
            raise ValueError(f"{1 << self.bits} levels are needed for {self.bits}-bit words, got {len(lv)}")
        if not all(np.isfinite(lv)):
            raise ValueError("levels must be finite")
        object.__setattr__(self, "levels", lv)
        object.__setattr__(self, "real", bool(self.real))

    @property
    def words_per_sample(self) -> int:
        return 1 if self.real else 2

    @property
    def sample_bits(self) -> int:
        return self.bits * self.words_per_sample

    def with_(self, **changes) -> "Packing":
        """A copy with some fields changed (e.g. `p.with_(order="lsb", real=True)`)."""
        d = dict(bits=self.bits, levels=self.levels, real=self.real, order=self.order)
        d.update(changes)
        return Packing(**d)

    def record(self) -> np.ndarray:
        """The gyp_packing record (numpy mirror _lib.PACKING, one element)."""
        r = np.zeros(1, dtype=_lib.PACKING)
        r["bits"], r["real"], r["order"] = self.bits, int(self.real), ORDERS[self.order]
        r["levels"][0, :len(self.levels)] = self.levels
        return r

    def file_samples(self, size_bytes: int) -> int:
        """Whole samples in a file of `size_bytes` bytes (trailing bits of a partial sample are ignored)."""
        return int(size_bytes) * 8 // self.sample_bits


def sign_magnitude(bits: int, real: bool = False, order: str = "msb") -> Packing:
    """Top bit the sign, the rest the magnitude: (1 - 2 s) (2 m + 1)."""
    h = 1 << (bits - 1)
    return Packing(bits, tuple((1 - 2 * (c >> (bits - 1))) * (2 * (c & (h - 1)) + 1) for c in range(1 << bits)), real, order)


def twos_complement(bits: int, real: bool = False, order: str = "msb") -> Packing:
    """c - 2^bits for c >= 2^(bits-1), else c."""
    return Packing(bits, tuple(c - (1 << bits) if c >= 1 << (bits - 1) else c for c in range(1 << bits)), real, order)


def offset_binary(bits: int, real: bool = False, order: str = "msb") -> Packing:
    """2 c - (2^bits - 1)."""
    return Packing(bits, tuple(2 * c - ((1 << bits) - 1) for c in range(1 << bits)), real, order)


PRESETS = {"sign_magnitude": sign_magnitude, "twos_complement": twos_complement, "offset_binary": offset_binary}


def pack(codes: Sequence[int], packing: Packing) -> bytes:
    """Codes (one per word, in file order: I, Q, I, Q, ... or real words) -> the packed bytes.  A last partial byte is padded
    with zero bits."""
    c = np.asarray(codes, dtype=np.int64).ravel()
    b = packing.bits
    if c.size and (c.min() < 0 or c.max() >= 1 << b):
        raise ValueError(f"codes must lie in [0, {1 << b})")
    per = 8 // b
    pad = (-c.size) % per
    c = np.concatenate([c, np.zeros(pad, dtype=np.int64)]).reshape(-1, per)
    slots = np.arange(per)
    shifts = 8 - b - b * slots if packing.order == "msb" else b * slots
    return (c << shifts).sum(axis=1).astype(np.uint8).tobytes()


def quantize(x: np.ndarray, packing: Packing, scale: float = 1.0) -> np.ndarray:
    """Real values (or complex ones, for an I,Q packing: interleaved I, Q words) -> the code of the nearest level to x / scale,
    ties to the lower code; int64 codes in file order."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        if packing.real:
            raise ValueError("a real packing takes real values")
        words = np.empty(2 * x.size, dtype=np.float64)
        words[0::2], words[1::2] = x.real.ravel(), x.imag.ravel()
    else:
        words = x.astype(np.float64).ravel()
    lv = np.asarray(packing.levels, dtype=np.float64)
    out = np.empty(words.size, dtype=np.int64)
    for i in range(0, words.size, 1 << 20):
        w = words[i:i + (1 << 20)] / float(scale)
        out[i:i + w.size] = np.argmin(np.abs(w[:, None] - lv[None, :]), axis=1)
    return out
