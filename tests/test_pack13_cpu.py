"""The lossless 13-bit bf16 packing as a format (no GPU): the numpy reference of
tests/_pack13.py round-trips every bf16 bit pattern, keeps raw exactly the rows the rule
names, and its byte count is the library's."""
import numpy as np
import pytest

import _pack13 as P


def _all_patterns_in_rows():
    """All 65,536 patterns, each in a row it is representable in: rows of one 15-step window
    of h (and h == 0, which every row represents), signs and low bytes in full."""
    rows = []
    for top in list(range(15, 128, 15)) + [127, 7]:
        hs = [h for h in range(max(1, top - 14), top + 1)] + [0]
        vals = [(s << 15) | (h << 8) | low for h in hs for s in (0, 1) for low in range(256)]
        rows.append(np.array(vals, dtype=np.uint16))
    width = max(len(r) for r in rows)
    out = np.zeros((len(rows), width), dtype=np.uint16)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
        out[i, len(r):] = r[-1]
    return out


def test_every_bit_pattern_round_trips():
    bits = _all_patterns_in_rows()
    assert len(np.unique(bits)) == 65536
    assert not P.unrepresentable(bits).any()
    low, sign, code, base = P.encode_rows(bits)
    assert code.max() == 15 and (base < 0).any()
    assert np.array_equal(P.decode_rows(low, sign, code, base), bits)


def test_raw_row_rule():
    K = 64
    row = np.full(K, (60 << 8) | 0x35, dtype=np.uint16)  # h = 60 everywhere
    ok = row.copy()
    ok[3] = (46 << 8) | 1      # h = top - 14: the lowest code
    ok[4] = 0x8000             # -0.0: h == 0 is always representable
    ok[5] = 0x007F             # a denormal
    bad = row.copy()
    bad[9] = (45 << 8) | 1     # h = top - 15 = base
    inf = row.copy()
    inf[0] = 0x7F80            # Inf counts like any value: top = 127, h = 60 is out
    zero = np.zeros(K, dtype=np.uint16)
    bits = np.stack([ok, bad, inf, zero, row, row])
    assert P.unrepresentable(bits).tolist() == [False, True, True, False, False, False]
    assert P.raw_rows(bits).tolist() == [True, True, True, True, False, False]
    assert P.raw_rows(bits, "gate_up").tolist() == [False, True, True, False, True, True]
    assert P.raw_rows(bits[:4], "head_halves", 4).tolist() == [True, True, True, True]
    hdr = P.headers(bits, P.raw_rows(bits))
    assert [int(h) >> 8 for h in hdr] == [1, 2, 3, 4, 0, 0]
    assert [((int(h) & 0xFF) ^ 0x80) - 0x80 for h in hdr] == [45, 45, 112, -15, 45, 45]


def test_planes_layout_round_trips():
    """The tile layout of pack_planes, read back value by value with the documented offsets."""
    rng = np.random.default_rng(5)
    N, K = 3, 2 * P.TILE
    h = rng.integers(50, 65, size=(N, K))
    bits = ((rng.integers(0, 2, size=(N, K)) << 15) | (h << 8)
            | rng.integers(0, 256, size=(N, K))).astype(np.uint16)
    bits[0, ::7] = 0
    planes = P.pack_planes(bits)
    assert planes.shape == (N, K // P.TILE * P.TILE_BYTES)
    base = P.row_top(bits) - 15
    for r, k in [(0, 0), (0, 7), (1, 13), (1, 2047), (2, 2048), (2, 4095), (0, 1000), (2, 3333)]:
        t, v = divmod(k, P.TILE)
        j, lane, e = v // 512, (v // 8) % 64, v % 8
        tile = planes[r, t * P.TILE_BYTES:(t + 1) * P.TILE_BYTES]
        low = tile[(j // 2) * 1024 + lane * 16 + (j % 2) * 8 + e]
        nib = 2 * e if e < 4 else 2 * (e - 4) + 1
        code = (tile[2048 + lane * 16 + j * 4 + nib // 2] >> (4 * (nib % 2))) & 15
        sign = (tile[3072 + lane * 4 + (e & 3)] >> (2 * j + (e >> 2))) & 1
        hh = 0 if code == 0 else base[r] + code
        assert (int(sign) << 15) | (int(hh) << 8) | int(low) == int(bits[r, k]), (r, k)


def test_normal_rows_rarely_need_the_fallback():
    """N(0, 0.02) rows of 4096 round-trip; the window of 15 codes is ~30 binades."""
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 4096, generator=g) * 0.02).to(torch.bfloat16)
    bits = w.view(torch.int16).numpy().view(np.uint16)
    assert int(P.unrepresentable(bits).sum()) <= 1
    keep = ~P.unrepresentable(bits)
    assert np.array_equal(P.decode_rows(*P.encode_rows(bits[keep])), bits[keep])


BYTES_CASES = [(1, 2048, 0), (6, 2048, 2), (130, 4096, 3), (128256, 4096, 11), (4096, 14336, 0),
               (8192, 28672, 5), (5, 1024, 0), (5, 2048 + 512, 0), (0, 2048, 0)]


@pytest.mark.parametrize("N,K,nraw", BYTES_CASES)
def test_bytes_formula(N, K, nraw):
    want = P.packed_bytes(N, K, nraw)
    if K % P.TILE == 0 and N > 0:
        assert want == N * K * 13 // 8 + (4 * N + 15) // 16 * 16 + 2 * nraw * K
    else:
        assert want == -1


@pytest.mark.parametrize("N,K,nraw", BYTES_CASES)
def test_bytes_formula_matches_the_library(N, K, nraw):
    from cake_amd.ops import _lib
    if not _lib.lib_path().exists():
        pytest.skip("the kernel library is not built")
    import ctypes as C
    lib = C.CDLL(str(_lib.lib_path()))
    lib.cake_pack13_bytes.restype = C.c_longlong
    assert int(lib.cake_pack13_bytes(C.c_int(N), C.c_int(K), C.c_int(nraw))) == P.packed_bytes(N, K, nraw)
