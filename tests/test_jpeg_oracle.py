"""The numpy JPEG oracle (tests/jpeg_np.py) against Pillow itself (libjpeg-turbo, the library
behind cv2.imread) where Pillow is importable, against the committed Pillow fixtures always, and
against known answers for the IDCT and the colour tables."""
import io

import numpy as np
import pytest

import jpeg_cases as C
import jpeg_np as J


def _pillow(img, **kw):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    data = b.getvalue()
    rgb = np.asarray(Image.open(io.BytesIO(data)))
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    return data, rgb, np.asarray(im)


def _same(data, rgb, y):
    got = J.decode(data, 1, keep_channel_order=True)
    assert np.array_equal(got if rgb.ndim == 3 else got[:, :, 0], rgb)
    assert np.array_equal(J.decode(data, 0), y)


@pytest.mark.parametrize("name", list(C.SAMPLINGS))
def test_grid_against_pillow(name):
    sub = {"gray": None, "444": 0, "422": 1, "420": 2}[name]
    for W in C.GRID_W:
        for H in C.GRID_H:
            img = J.test_image(W * 100 + H, H, W, 1 if sub is None else 3)
            kw = {} if sub is None else {"subsampling": sub}
            _same(*_pillow(img, quality=75, **kw))


@pytest.mark.parametrize("name", list(C.SAMPLINGS))
def test_97x131_against_pillow(name):
    sub = {"gray": None, "444": 0, "422": 1, "420": 2}[name]
    for q, extra in ((30, {}), (75, {"optimize": True}), (95, {"restart_marker_blocks": 5})):
        img = J.test_image(q, 131, 97, 1 if sub is None else 3)
        kw = dict(extra) if sub is None else dict(extra, subsampling=sub)
        _same(*_pillow(img, quality=q, **kw))


def test_committed_fixtures():
    fx = C.pillow_fixtures()
    assert len(fx) >= 12
    for name, (data, rgb, y) in fx.items():
        _same(data, rgb, y)


def test_own_writer_round_trip_and_info():
    img = J.test_image(4, 37, 45, 3)
    for samp, sub in (((1, 1), 444), ((2, 1), 422), ((2, 2), 420)):
        data = J.encode_image(img, 90, samp, ri=2)
        assert J.info(data) == (37, 45, 3, sub)
        assert J.decode(data, 1).shape == (37, 45, 3) and J.decode(data, 0).shape == (37, 45)
    assert J.info(J.encode_image(img[:, :, 0])) == (37, 45, 1, 0)


def test_idct_known_answers():
    q = np.ones(64, np.int64)
    c = np.zeros(64, np.int16)
    for dc, want in ((0, 128), (8, 129), (-8, 127), (800, 228), (2000, 255), (-2000, 0), (4, 129), (-4, 128), (3, 128)):
        c[0] = dc
        assert (J.idct_blocks(c[None], q)[0] == want).all(), dc
    # one AC coefficient each: the float inverse DCT within one level, symmetric / antisymmetric
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    basis[0] /= np.sqrt(2)
    for idx in range(1, 64):
        c[:] = 0
        c[idx] = 64
        got = J.idct_blocks(c[None], q)[0].astype(int)
        ref = 128 + 64 * np.outer(basis[idx // 8], basis[idx % 8])
        assert np.abs(got - ref).max() <= 1, idx
    c[:] = 0
    c[0], c[1], c[8] = 1023, 1023, -1023            # saturates both ways
    got = J.idct_blocks(c[None], q)[0]
    assert got.min() == 0 and got.max() == 255
    assert np.array_equal(J.idct_blocks(c[None], q * 2), J.idct_blocks((c * 2)[None], q))


def test_colour_tables_closed_form():
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for y in (0, 128, 255):
        r, g, b = J.ycc_to_rgb(np.full_like(cb, y), cb, cr)
        fr = y + 1.402 * (cr - 128)
        fg = y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128)
        fb = y + 1.772 * (cb - 128)
        for got, f in ((r, fr), (g, fg), (b, fb)):
            assert np.abs(got.astype(float) - np.clip(f, 0, 255)).max() <= 0.51
        assert r[0, 128] == g[128, 128] == b[128, 0] == y
    for v, want in ((128, 0), (255, 178), (0, -179)):
        assert (91881 * (v - 128) + 32768) >> 16 == want
