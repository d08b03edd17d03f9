"""The PLY row formatter against Python's own '%f' / '%d' (np.savetxt, the call of
io_functions.write_ply), byte for byte, on a machine without a GPU: sm_ply_format_host runs the
row function the kernels run (sm_cloud.hpp ply_row) on the CPU and needs no context.

Every generated value is compared: each test formats the whole array and compares the whole body."""
import io

import numpy as np
import pytest

import stereo_match_amd as sma
from stereo_match_amd import _lib

FMT = '%f %f %f %d %d %d '


def savetxt_body(verts, colors) -> bytes:
    f = io.BytesIO()
    np.savetxt(f, np.hstack([verts, colors]), fmt=FMT)
    return f.getvalue()


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def special_values() -> np.ndarray:
    """The cases DESIGN.md §4.9 lists, as float32."""
    nxt = lambda x, d: np.nextafter(np.float32(x), np.float32(d))  # noqa: E731
    flt_max = np.finfo(np.float32).max
    v = [
        np.float32(1 / 128), np.float32(3 / 128),           # ties to even: 0.007812, 0.023438
        np.float32(0.99999994),                              # the carry: 1.000000
        np.float32(0.0), np.float32(-0.0),                   # -0.000000
        f32(0x00000001), f32(0x80000001),                    # +-smallest denormal (negative underflow)
        flt_max, -flt_max,                                   # 39 digits
        np.float32(np.inf), np.float32(-np.inf),
        f32(0x7FC00000), f32(0xFFC00000), f32(0x7F800001), f32(0xFFFFFFFF),  # nan is never signed
        np.float32(2.0 ** 24), nxt(2.0 ** 24, 0), nxt(2.0 ** 24, np.inf),
        np.float32(2.0 ** 64), nxt(2.0 ** 64, 0), nxt(2.0 ** 64, np.inf),
        np.float32(1e10), np.float32(-123456.789),
        np.float32(0.5e-6), np.float32(1.5e-6), np.float32(-0.5e-6),  # around half a unit of the sixth decimal
        np.float32(999999.9375), np.float32(9.9999995), np.float32(2.0 ** 40), np.float32(2.0 ** 41),
        np.float32(2.0 ** 63), np.float32(2.0 ** 96), np.float32(2.0 ** 127),
    ]
    v = np.array([np.float32(x) for x in v], np.float32)
    return v


def rows_of(values: np.ndarray, seed=0):
    """Pad to a multiple of 3 with 0 and give every row colours."""
    n = (len(values) + 2) // 3
    v = np.zeros(3 * n, np.float32)
    v[:len(values)] = values
    rng = np.random.default_rng(seed)
    return v.reshape(n, 3), rng.integers(0, 256, (n, 3), dtype=np.uint8)


def check(verts, colors):
    got = sma.format_ply(verts, colors)
    want = savetxt_body(verts, colors)
    if got != want:  # name the first row that differs
        g, w = got.split(b"\n"), want.split(b"\n")
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"row {i}: {a!r} != {b!r} (bits {verts[i].view(np.uint32)})"
        assert len(g) == len(w)
    assert got == want


def test_special_values_known_text():
    v = np.array([[1 / 128, 3 / 128, 0.99999994], [-0.0, np.inf, -np.inf]], np.float32)
    v = np.vstack([v, [f32(0xFFC00000), f32(0x80000001), np.float32(3.4028235e38)]]).astype(np.float32)
    c = np.array([[0, 9, 10], [99, 100, 255], [1, 2, 3]], np.uint8)
    assert sma.format_ply(v, c) == (
        b"0.007812 0.023438 1.000000 0 9 10 \n"
        b"-0.000000 inf -inf 99 100 255 \n"
        b"nan -0.000000 340282346638528859811704183484516925440.000000 1 2 3 \n")


def test_special_values_match_python():
    sp = special_values()
    assert np.isnan(sp).sum() == 4 and np.isinf(sp).sum() == 2
    check(*rows_of(sp))
    # every special value in every column
    for shift in (1, 2):
        check(*rows_of(np.concatenate([np.zeros(shift, np.float32), sp])))


def test_all_odd_ties_over_128():
    t = np.arange(1, 4096, 2, dtype=np.float32) / np.float32(128)
    assert len(t) == 2048
    check(*rows_of(np.concatenate([t, -t])))


def test_random_bit_patterns():
    rng = np.random.default_rng(20240)
    bits = rng.integers(0, 1 << 32, 300_000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    assert np.isnan(v).any() and (((bits >> 23) & 0xFF) == 0).any()  # NaNs and denormals are in
    check(*rows_of(v, seed=1))


def test_typical_coordinate_range():
    rng = np.random.default_rng(7)
    n = 300_000
    v = np.exp(rng.uniform(np.log(1e-3), np.log(1e6), n)).astype(np.float32)
    v[::2] *= -1
    assert np.abs(v).min() >= np.float32(1e-3) * 0.999 and np.abs(v).max() <= 1e6
    check(*rows_of(v, seed=2))


def test_every_colour_value_in_every_column():
    c = np.stack([np.arange(256), np.roll(np.arange(256), 85), np.roll(np.arange(256), 170)], 1).astype(np.uint8)
    for col in range(3):
        assert sorted(c[:, col].tolist()) == list(range(256))
    v = np.linspace(-3, 3, 768, dtype=np.float32).reshape(256, 3)
    check(v, c)


def test_empty():
    v, c = np.empty((0, 3), np.float32), np.empty((0, 3), np.uint8)
    assert sma.format_ply(v, c) == b""
    assert _lib.ply_format_host(v, c).size == 0


def test_capacity_too_small_is_reported_and_nothing_written():
    import ctypes

    v, c = rows_of(special_values())
    want = savetxt_body(v, c)
    lib = _lib.load()
    nb = ctypes.c_uint64()
    for cap in (0, 1, len(want) // 2, len(want) - 1):
        buf = np.full(len(want) + 64, 0xAB, np.uint8)
        rc = lib.sm_ply_format_host(v.ctypes.data, c.ctypes.data, len(v), cap, buf.ctypes.data, ctypes.byref(nb))
        assert rc == _lib.SM_E_ARG and nb.value == len(want)
        assert (buf == 0xAB).all()
        with pytest.raises(ValueError, match="capacity"):
            _lib.ply_format_host(v, c, capacity=cap)
    # the exact capacity fits, and the bytes behind it stay untouched
    buf = np.full(len(want) + 64, 0xAB, np.uint8)
    rc = lib.sm_ply_format_host(v.ctypes.data, c.ctypes.data, len(v), len(want), buf.ctypes.data, ctypes.byref(nb))
    assert rc == _lib.SM_OK and nb.value == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()


def test_longest_row_is_157_bytes():
    v = np.full((1, 3), -np.finfo(np.float32).max, np.float32)
    c = np.full((1, 3), 255, np.uint8)
    assert len(sma.format_ply(v, c)) == _lib.PLY_MAX_ROW == 157
    check(v, c)


def test_multithreaded_chunks_join_in_order():
    """More rows than one chunk of the host formatter: the chunks' offsets."""
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((200_000, 3)) * 100).astype(np.float32)
    c = rng.integers(0, 256, (200_000, 3), dtype=np.uint8)
    check(v, c)


def test_format_ply_refuses_other_dtypes():
    v = np.zeros((2, 3), np.float64)
    c = np.zeros((2, 3), np.uint8)
    with pytest.raises(ValueError, match="write_ply"):
        sma.format_ply(v, c)
    with pytest.raises(ValueError, match="write_ply"):
        sma.format_ply(v.astype(np.float32), c.astype(np.int32))
    with pytest.raises(ValueError, match="write_ply"):
        sma.format_ply(np.zeros((2, 4), np.float32), np.zeros((2, 4), np.uint8))
