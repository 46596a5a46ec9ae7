"""Numpy reference of the lossless 13-bit bf16 packing (csrc/kernels/gemv_p13_kernel.h),
written from the format's definition, not from the kernels: per value the low byte, the sign
and a 4-bit code = h - base (h = the exponent's upper 7 bits, base = the row's largest h - 15;
code 0 keeps h == 0), rows with a value of 0 < h <= base kept raw, and the planar tile layout."""
import numpy as np

TILE, TILE_BYTES = 2048, 3328
KINDS = {"adjacent": 0, "head_halves": 1, "gate_up": 2}


def packed_bytes(N: int, K: int, nraw: int) -> int:
    """planes | headers (padded to 16 bytes) | raw rows; -1: K is not whole tiles."""
    if N < 1 or K < TILE or K % TILE or nraw < 0:
        return -1
    return N * (K // TILE) * TILE_BYTES + (4 * N + 15) // 16 * 16 + nraw * K * 2


def row_top(bits: np.ndarray) -> np.ndarray:
    """bits uint16 [N, K] -> the largest h of every row (Inf and NaN count like any value)."""
    return ((bits >> 8) & 0x7F).astype(np.int64).max(axis=1)


def unrepresentable(bits: np.ndarray) -> np.ndarray:
    """bool [N]: the row has a value with 0 < h <= base."""
    h = ((bits >> 8) & 0x7F).astype(np.int64)
    base = row_top(bits)[:, None] - 15
    return ((h > 0) & (h <= base)).any(axis=1)


def partner(kind: str, r: int, N: int, hd: int = 0) -> int:
    if kind == "head_halves":
        return r + hd // 2 if r % hd < hd // 2 else r - hd // 2
    if kind == "gate_up":
        return r + N // 2 if r < N // 2 else r - N // 2
    return r ^ 1 if (r ^ 1) < N else r


def raw_rows(bits: np.ndarray, kind: str = "adjacent", hd: int = 0) -> np.ndarray:
    """bool [N]: rows kept raw — unrepresentable, or paired with one that is."""
    u = unrepresentable(bits)
    N = len(u)
    return np.array([u[r] or u[partner(kind, r, N, hd)] for r in range(N)])


def encode_rows(bits: np.ndarray):
    """(low uint8, sign uint8, code uint8 [N, K], base int [N]) of representable rows."""
    h = ((bits >> 8) & 0x7F).astype(np.int64)
    base = row_top(bits) - 15
    code = np.where(h == 0, 0, h - base[:, None])
    assert code.min() >= 0 and code.max() <= 15
    return (bits & 0xFF).astype(np.uint8), (bits >> 15).astype(np.uint8), code.astype(np.uint8), base


def decode_rows(low, sign, code, base) -> np.ndarray:
    h = np.where(code == 0, 0, base[:, None] + code.astype(np.int64))
    return (sign.astype(np.uint16) << 15) | (h.astype(np.uint16) << 8) | low.astype(np.uint16)


def pack_planes(bits: np.ndarray) -> np.ndarray:
    """The planes uint8 [N, K / 2048 * 3328] of representable rows, in the tile layout: lane l
    of a tile owns its 16-bit chunks l + 64 j (8 values each, j < 4)."""
    N, K = bits.shape
    low, sign, code, _ = encode_rows(bits)
    T = K // TILE
    shape = (N, T, 4, 64, 8)  # [row, tile, j, lane, e]
    low, sign, code = low.reshape(shape), sign.reshape(shape), code.reshape(shape)
    lows = np.zeros((N, T, 2, 64, 2, 8), dtype=np.uint8)  # [half plane, lane, j & 1, e]
    for j in range(4):
        lows[:, :, j // 2, :, j % 2, :] = low[:, :, j]
    codes = np.zeros((N, T, 64, 4, 4), dtype=np.uint8)  # [lane, j, byte]
    signs = np.zeros((N, T, 64, 4), dtype=np.uint8)  # [lane, byte]
    for j in range(4):
        for e in range(8):
            nib = 2 * e if e < 4 else 2 * (e - 4) + 1
            codes[:, :, :, j, nib // 2] |= code[:, :, j, :, e] << (4 * (nib % 2))
            signs[:, :, :, e & 3] |= sign[:, :, j, :, e] << (2 * j + (e >> 2))
    out = np.concatenate([lows.reshape(N, T, 2048), codes.reshape(N, T, 1024),
                          signs.reshape(N, T, 256)], axis=2)
    return out.reshape(N, T * TILE_BYTES)


def headers(bits: np.ndarray, raw: np.ndarray) -> np.ndarray:
    """int32 [N]: (slot + 1) << 8 | (base & 0xff), the raw rows' slots in row order."""
    slot = np.where(raw, np.cumsum(raw), 0)
    return ((slot << 8) | ((row_top(bits) - 15) & 0xFF)).astype(np.int32)
