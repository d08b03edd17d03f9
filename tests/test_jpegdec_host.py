"""The JPEG decoder's CPU twin (sm_jpeg_decode_host, a plain serial decoder built from the
functions the kernels run) against the numpy oracle and the committed Pillow fixtures; every
refusal and corruption class by message and code; the dispatch in png.py."""
import numpy as np
import pytest

import jpeg_cases as C
import jpeg_np as J
import png_np
import stereo_match_amd as sm
from stereo_match_amd import _lib


def same(data, flags=(1, 0, -1)):
    for fl in flags:
        got = sm.imdecode_host(data, fl)
        assert got.dtype == np.uint8 and np.array_equal(got, J.decode(data, fl)), fl
    assert _lib.jpeg_info(data) == J.info(data)
    assert _lib.jpeg_decode_stats(None) == (C.n_subsequences(data), 0)


@pytest.mark.parametrize("name", list(C.SAMPLINGS))
def test_geometry_grid(name):
    samp = C.SAMPLINGS[name]
    for W in C.GRID_W:
        for H in C.GRID_H:
            same(C.grid_file(samp, W, H, ri=(W + H) % 3), flags=(1, 0))


@pytest.mark.parametrize("name", list(C.SAMPLINGS))
def test_97x131_three_qualities(name):
    samp = C.SAMPLINGS[name]
    for q, ri in ((30, 0), (75, 7), (95, 1)):
        img = J.test_image(q, 131, 97, 1 if samp is None else 3)
        same(J.encode_image(img, q, samp or (1, 1), ri))


def test_pillow_fixtures():
    for name, (data, rgb, y) in C.pillow_fixtures().items():
        got = sm.imdecode_host(data, 1, keep_channel_order=True)
        assert np.array_equal(got if rgb.ndim == 3 else got[:, :, 0], rgb), name
        assert np.array_equal(sm.imdecode_host(data, 0), y), name
        assert np.array_equal(sm.imdecode_host(data, 1), got[:, :, ::-1]), name


@pytest.mark.parametrize("name", list(C.handmade()))
def test_handmade_streams(name):
    same(C.handmade()[name])


def test_structured_scans():
    for data in (C.scan_of_length(100), C.scan_of_length(C.SUBSEQ), C.scan_of_length(2 * C.SUBSEQ), C.scan_of_lanes(65),
                 C.stuffing_file(), C.interval_of_length(C.SUBSEQ + 1), C.identical_blocks()):
        same(data, flags=(1,))


@pytest.mark.parametrize("name", list(C.faulty()))
def test_refusals_and_corruptions(name):
    data, code, text = C.faulty()[name]
    with pytest.raises(sm.SmError) as e:
        sm.imdecode_host(data, 1)
    assert e.value.code == code and text in str(e.value), str(e.value)
    with pytest.raises(J.JpegError) as o:
        J.decode(data, 1)
    assert o.value.code == code


def test_truncation_at_every_length_is_refused():
    data = C.grid_file((2, 2), 17, 9, ri=1)
    for n in range(3, len(data)):
        with pytest.raises(sm.SmError) as e:
            sm.imdecode_host(data[:n], 1)
        assert e.value.code == _lib.SM_E_DATA, n


def test_dispatch_leaves_png_alone():
    img = png_np.runny(3, (9, 11, 3))
    png = sm.imencode_png_host(img)
    assert np.array_equal(sm.imdecode_host(png, 1), img)
    for junk in (b"\xff\xd8garbage", b"\xff\xd8\xff\x00garbage", b"\xff\xd8"):
        with pytest.raises(sm.SmError) as e:
            sm.imdecode_host(junk, 1)
        assert e.value.code == _lib.SM_E_DATA
    with pytest.raises(sm.SmError, match="not a PNG file"):
        sm.imdecode_host(b"GIF89a" + bytes(40), 1)
    with pytest.raises(ValueError):
        sm.imdecode_host(C.grid_file(None, 8, 8), 2)


def test_status_table_and_descriptor():
    lib = _lib.load()
    codes = [lib.sm_jpegdec_status_code(s) for s in range(1, 27)]
    assert set(codes) == {_lib.SM_E_DATA, _lib.SM_E_UNSUPPORTED}
    assert all(lib.sm_jpegdec_status_message(s).decode().startswith("unsupported") == (c == _lib.SM_E_UNSUPPORTED)
               for s, c in zip(range(1, 27), codes))
    assert lib.sm_jpegdec_status_code(0) == 0 and lib.sm_jpegdec_status_message(99) == b"unknown status"
    assert _lib.jpeg_parse(C.grid_file((2, 2), 16, 16)).size == lib.sm_jpeg_desc_bytes()
