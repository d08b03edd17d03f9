"""The JPEG decoder on the device (sm_jpegdec.hpp: k_jpeg_split, _sync_a, _sync_b, _sync_loop,
_write, _dc, _idct, _color): its pixels and status against the CPU twin's and against the numpy
oracle (tests/jpeg_np.py), its lane count against the scan's structure."""
import numpy as np
import pytest

import jpeg_cases as C
import jpeg_np as J
import stereo_match_amd as sm
from stereo_match_amd import _lib, jpeg as smjpeg

pytestmark = pytest.mark.gpu


def check(data, flags=(1,), oracle=True, min_rounds=None):
    """device == host twin == oracle for every flag; the device's lane count is the scan's"""
    lanes = C.n_subsequences(data)
    for fl in flags:
        host = sm.imdecode_host(data, fl)
        assert _lib.jpeg_decode_stats(None) == (lanes, 0)
        dev = sm.imdecode(data, fl)
        assert dev.dtype == host.dtype and dev.shape == host.shape
        assert np.array_equal(dev, host), f"flags {fl}: device != host twin"
        nsub, rounds = _lib.engine(0).jpeg_decode_stats()
        assert nsub == lanes, (nsub, lanes)
        assert rounds <= lanes and (lanes > 1 or rounds == 0), (rounds, lanes)
        if min_rounds is not None:
            assert rounds >= min_rounds, (rounds, min_rounds)
        if oracle:
            assert np.array_equal(dev, J.decode(data, fl)), f"flags {fl}: device != oracle"


@pytest.mark.parametrize("name", list(C.SAMPLINGS))
def test_geometry_grid(name):
    samp = C.SAMPLINGS[name]
    for W in C.GRID_W:
        for H in C.GRID_H:
            check(C.grid_file(samp, W, H, ri=(W + H) % 3), flags=(1, 0) if (W + H) % 4 == 0 else (1,))


def test_pillow_fixtures():
    for name, (data, rgb, y) in C.pillow_fixtures().items():
        got = sm.imdecode(data, 1, keep_channel_order=True)
        want = rgb if rgb.ndim == 3 else np.repeat(rgb[:, :, None], 3, axis=2)
        assert np.array_equal(got, want), name
        assert np.array_equal(sm.imdecode(data, 0), y), name
        check(data, flags=(1,))


@pytest.mark.parametrize("what", ["short", "one", "two", "wave", "many"])
def test_sub_sequence_structure(what):
    data = {"short": lambda: C.scan_of_length(100), "one": lambda: C.scan_of_length(C.SUBSEQ),
            "two": lambda: C.scan_of_length(2 * C.SUBSEQ), "wave": lambda: C.scan_of_lanes(65),
            "many": lambda: C.scan_of_lanes(300)}[what]()
    assert C.n_subsequences(data) == {"short": 1, "one": 1, "two": 2, "wave": 65, "many": 300}[what]
    check(data)


def test_cut_on_a_stuffed_byte_and_before_rst():
    data = C.stuffing_file()
    assert C.cut_on_stuffing(data)
    check(data)
    data = C.interval_of_length(C.SUBSEQ + 1)
    assert J.scan_intervals(data)[0][0][1] - J.scan_intervals(data)[0][0][0] == C.SUBSEQ + 1
    check(data)


def test_restart_interval_of_one_mcu_and_of_a_row():
    img = J.test_image(3, 40, 72, 3)
    check(J.encode_image(img, 85, (2, 2), ri=1), flags=(1, 0))
    check(J.encode_image(img, 85, (2, 1), ri=5))          # a row of 16-wide MCUs
    check(J.encode_image(img[:, :, 1], 85, ri=9))


def test_identical_blocks_need_synchronisation_rounds():
    data = C.identical_blocks()
    assert C.n_subsequences(data) > 4
    check(data, min_rounds=1)
    print("identical blocks: (lanes, rounds) =", _lib.engine(0).jpeg_decode_stats())


@pytest.mark.parametrize("name", list(C.handmade()))
def test_handmade_streams(name):
    check(C.handmade()[name], flags=(1, 0, -1))


def test_flags_channel_order_and_tensors():
    import torch

    colour = C.grid_file((2, 2), 33, 31)
    gray = C.grid_file(None, 33, 31)
    for data in (colour, gray):
        for fl in (1, 0, -1):
            want = J.decode(data, fl)
            assert np.array_equal(sm.imdecode(data, fl), want)
            t = sm.imdecode(data, fl, as_tensor=True)
            assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want)
    assert sm.imdecode(colour, -1).shape == (31, 33, 3) and sm.imdecode(gray, -1).shape == (31, 33)
    rgb = sm.imdecode(colour, 1, keep_channel_order=True)
    assert np.array_equal(rgb, J.decode(colour, 1)[:, :, ::-1])


def test_imread(tmp_path):
    data = C.grid_file((2, 1), 17, 9)
    path = str(tmp_path / "frame.jpeg")
    with open(path, "wb") as f:
        f.write(data)
    assert np.array_equal(sm.imread(path), J.decode(data, 1))
    assert np.array_equal(sm.imread(path, 0), J.decode(data, 0))
    assert sm.imread(str(tmp_path / "missing.jpg")) is None


def test_batch_of_one_geometry_and_mixed_batch():
    img = J.test_image(8, 45, 52, 3)
    coefs, qts = J.image_coefficients(img, 80, (2, 2))
    files = [J.encode_image(img, 80, (2, 2)), J.encode_image(img, 30, (2, 2), ri=1), J.encode_image(img, 95, (2, 2), ri=4),
             J.write_jpeg(coefs, qts, 45, 52, (2, 2), ri=2, ac_tables=[J.default_table(J.ac_symbols(), first_len=3)] * 2),
             J.encode_image(img[::-1].copy(), 80, (2, 2), ri=3)]
    out = sm.imdecode_batch(files, 1)
    assert out.is_cuda and tuple(out.shape) == (5, 45, 52, 3)
    for i, f in enumerate(files):
        assert np.array_equal(out[i].cpu().numpy(), J.decode(f, 1)), i
    assert _lib.engine(0).jpeg_decode_stats()[0] == sum(C.n_subsequences(f) for f in files)
    y = sm.imdecode_batch(files, 0)
    assert np.array_equal(y[1].cpu().numpy(), J.decode(files[1], 0))
    with pytest.raises(sm.SmError, match="image 2: geometry") as e:
        sm.imdecode_batch(files[:2] + [J.encode_image(img, 80, (2, 1))], 1)
    assert e.value.code == _lib.SM_E_UNSUPPORTED
    bad = C.faulty()["bad_code"][0]
    with pytest.raises(sm.SmError, match="image 1: .*in no table"):
        sm.imdecode_batch([J.encode_image(J.test_image(11, 24, 40, 3), 75, (1, 1)), bad], 1)


@pytest.mark.parametrize("name", C.DEVICE_FAULTY)
def test_named_corrupt_files(name):
    data, code, text = C.faulty()[name]
    with pytest.raises(sm.SmError) as host:
        sm.imdecode_host(data, 1)
    with pytest.raises(sm.SmError) as dev:
        sm.imdecode(data, 1)
    assert text in str(dev.value) and dev.value.code == host.value.code == code
    assert str(dev.value) == str(host.value)


def test_strided_output_into_a_slice():
    import torch

    data = C.grid_file((2, 2), 33, 17)
    big = torch.full((2, 17, 50, 3), 7, dtype=torch.uint8, device="cuda")
    view = big[1:2, :, 10:43, :]
    smjpeg.decode_batch_device([np.frombuffer(data, np.uint8)], 1, 0, out=view)
    assert np.array_equal(view[0].cpu().numpy(), J.decode(data, 1))
    untouched = big.clone()
    untouched[1:2, :, 10:43, :] = 7
    assert bool((untouched == 7).all())


def test_jpeg_frames_into_the_matcher():
    rng = np.random.RandomState(5)
    base = np.clip(rng.normal(128, 60, (64, 104)), 0, 255).astype(np.uint8)
    left = np.repeat(base[:, 8:, None], 3, axis=2)
    right = np.repeat(base[:, :96, None], 3, axis=2)
    files = [J.encode_image(left, 95, (2, 2)), J.encode_image(right, 95, (2, 2), ri=3)]
    frames = sm.imdecode_batch(files, 1)
    assert tuple(frames.shape) == (2, 64, 96, 3)
    m = sm.StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=5)
    dt = m.compute(sm.cvtColor(frames[0]), sm.cvtColor(frames[1]))
    gl, gr = sm.cvtColor(J.decode(files[0], 1)), sm.cvtColor(J.decode(files[1], 1))
    dn = m.compute(gl, gr)
    assert dt.is_cuda and np.array_equal(dt.cpu().numpy(), dn)
