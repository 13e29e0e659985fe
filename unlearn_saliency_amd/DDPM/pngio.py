"""A PNG writer on the standard library: 8-bit RGB (or greyscale), filter type 0 on every row, one IDAT chunk.  It is all
the sampler needs — the images come off the device as uint8 (H, W, C) arrays (ops_sampler.images_to_u8) — and keeps
the package free of an imaging dependency on the writing side; any PNG reader opens the files."""
from __future__ import annotations

import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_COLOR_TYPE = {1: 0, 3: 2}  # channels -> PNG colour type (greyscale, truecolour)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(img: np.ndarray, level: int = 6) -> bytes:
    """img: uint8 (H, W, 3) or (H, W, 1) / (H, W)."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"encode_png needs uint8 pixels, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in _COLOR_TYPE or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_png needs (H, W, 3) or (H, W, 1) pixels, got {a.shape}")
    h, w, c = a.shape
    rows = np.zeros((h, 1 + w * c), dtype=np.uint8)  # a filter byte 0 in front of every row
    rows[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, _COLOR_TYPE[c], 0, 0, 0)
    return _SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path: str, img: np.ndarray, level: int = 6) -> None:
    with open(path, "wb") as f:
        f.write(encode_png(img, level))


def image_grid(imgs: np.ndarray, nrow: int) -> np.ndarray:
    """(N, H, W, C) -> one (ceil(N / nrow) * H, nrow * W, C) image, `nrow` tiles per row, no padding between tiles
    (torchvision's make_grid(nrow=nrow, padding=0)); missing tiles of the last row stay black."""
    n, h, w, c = imgs.shape
    ncol = min(nrow, n)
    nr = (n + ncol - 1) // ncol
    full = np.zeros((nr * ncol, h, w, c), dtype=imgs.dtype)
    full[:n] = imgs
    return full.reshape(nr, ncol, h, w, c).transpose(0, 2, 1, 3, 4).reshape(nr * h, ncol * w, c)
