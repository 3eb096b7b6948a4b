"""A numpy model of packed recordings (include/gypsum_hip.h, "packed recordings"): unpacking by the contract's bit arithmetic,
word by word, and the span of bytes a block of samples reads.  Independent of gypsum_amd.packing.pack, which it checks."""
from __future__ import annotations

import numpy as np


def unpack_codes(data: bytes, bits: int, order: str, n_words: int | None = None) -> np.ndarray:
    """The codes of words 0 .. n_words-1 (default: every whole word) of a byte stream: word w is bits [w*bits, (w+1)*bits),
    byte (w*bits) // 8; within the byte the earliest word is the most significant ("msb") or the least ("lsb")."""
    b = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    total = len(b) * 8 // bits
    n = total if n_words is None else int(n_words)
    w = np.arange(n, dtype=np.int64)
    pos = w * bits
    byte = b[pos // 8]
    slot = pos % 8
    shift = 8 - bits - slot if order == "msb" else slot
    return (byte >> shift) & ((1 << bits) - 1)


def unpack_values(data: bytes, bits: int, order: str, levels, real: bool, scale: float = 1.0) -> np.ndarray:
    """Every whole sample's value in float32 (levels[code] * float32(scale), one float32 multiply): complex64 for I,Q, float32
    for real."""
    wps = 1 if real else 2
    n = len(data) * 8 // (bits * wps)
    codes = unpack_codes(data, bits, order, n * wps)
    v = np.asarray(levels, dtype=np.float32)[codes] * np.float32(scale)
    return v if real else (v[0::2] + 1j * v[1::2]).astype(np.complex64)


def span(bits: int, real: bool, file_bytes: int, first: int, n: int, samples_per_ms: int) -> dict:
    """gyp_packed_span by brute force: the samples of [first, first + n) inside the file, the bytes their bits touch."""
    B = bits * (1 if real else 2)
    file_samples = file_bytes * 8 // B
    inside = [s for s in range(max(first, 0), min(first + n, file_samples))]
    total_ms = (file_samples - 1) // samples_per_ms if file_samples > 0 else 0
    if not inside:
        return dict(in_first=0, in_n=0, first_byte=0, bit0=0, n_bytes=0, file_samples=file_samples, total_ms=total_ms)
    touched = {bit // 8 for s in (inside[0], inside[-1]) for bit in range(s * B, (s + 1) * B)}
    return dict(in_first=inside[0], in_n=len(inside), first_byte=min(touched), bit0=inside[0] * B - 8 * min(touched),
                n_bytes=max(touched) - min(touched) + 1, file_samples=file_samples, total_ms=total_ms)
