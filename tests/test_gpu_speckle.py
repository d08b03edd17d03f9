"""The speckle filter (csrc/sm_speckle.hpp, a lock-free union-find) on the shapes that are hard for
one, against oracle/sgm_np.filter_speckles, bit-exact: one long corridor, one region filling the
image, combs, ramps that connect by chain only, regions of exactly maxsize and maxsize + 1 pixels,
the ends of int16, images of one row or one column, and a batch of different images."""
import functools

import numpy as np
import pytest

from oracle import sgm_np
from stereo_match_amd import _lib

pytestmark = pytest.mark.gpu

NEW = -16


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _oracle(data, shape, newval, maxsize, maxdiff):
    out = sgm_np.filter_speckles(np.frombuffer(data, np.int16).reshape(shape), newval, maxsize, maxdiff)
    out.setflags(write=False)
    return out


def oracle(img, newval, maxsize, maxdiff):
    return _oracle(img.tobytes(), img.shape, newval, maxsize, maxdiff)


def check(eng, img, newval, maxsize, maxdiff, changed=None):
    """The device against the oracle; `changed`: how many pixels the oracle itself must change."""
    exp = oracle(img, newval, maxsize, maxdiff)
    if changed is not None:
        assert int((exp != img).sum()) == changed, "the case does not do what it is there for"
    got = eng.filter_speckles(img, newval, maxsize, maxdiff)
    bad = np.argwhere(got != exp)
    assert not len(bad), f"{len(bad)} px differ, first at {tuple(bad[0])} (maxsize {maxsize}, maxdiff {maxdiff})"
    return got


def serpentine(H=64, W=64, newval=NEW):
    """One corridor through the whole image: the even rows, joined at alternating ends by one
    pixel of each odd row (the last odd row's pixel is a dead end).  The values vary within
    maxdiff 2, in runs of three along a row."""
    yy, xx = np.mgrid[:H, :W]
    img = (400 + (xx // 3 + yy) % 3).astype(np.int16)
    for y in range(1, H, 2):
        keep = W - 1 if y % 4 == 1 else 0
        row = img[y].copy()
        img[y] = newval
        img[y, keep] = row[keep]
    return img


def uniform(H=96, W=130):
    return np.full((H, W), 320, np.int16)


def checkerboard(H, W, step):
    yy, xx = np.mgrid[:H, :W]
    return (160 + step * ((xx + yy) & 1)).astype(np.int16)


def comb(H=64, W=64, joined=True, newval=NEW):
    """One-pixel teeth in the even columns, of lengths that differ, over a joining bottom row."""
    img = np.full((H, W), newval, np.int16)
    for x in range(0, W, 2):
        img[x % 7:H - 1, x] = 240 + x % 5
    if joined:
        img[H - 1] = 242
    return img


def blocky(H, W, seed, newval=NEW, holes=0.1):
    rng = np.random.default_rng(seed)
    img = (rng.integers(0, 6, (H // 3 + 1, W // 2 + 1)) * 40).astype(np.int16)
    img = np.ascontiguousarray(np.kron(img, np.ones((3, 2), np.int16))[:H, :W])
    img[rng.random(img.shape) < holes] = newval
    return img


def region_size(img, newval=NEW):
    return int((img != newval).sum())


# ---- long chains
@pytest.mark.parametrize("transposed", [False, True])
def test_serpentine(eng, transposed):
    img = serpentine()
    if transposed:
        img = np.ascontiguousarray(img.T)
    n = region_size(img)
    assert n == 32 * 64 + 32
    check(eng, img, NEW, n - 1, 2, changed=0)
    check(eng, img, NEW, n, 2, changed=n)
    check(eng, img, NEW, n + 1, 2, changed=n)
    # maxdiff 0 cuts the corridor into the runs of three, and what is left over of a row
    got = check(eng, img, NEW, 2, 0)
    assert 0 < int((got != img).sum()) < n


def test_uniform(eng):
    img = uniform()
    n = img.size
    check(eng, img, NEW, n - 1, 0, changed=0)
    check(eng, img, NEW, n, 0, changed=n)


@pytest.mark.parametrize("H,W", [(64, 64), (33, 127)])
def test_checkerboard(eng, H, W):
    maxdiff = 16
    split = checkerboard(H, W, maxdiff + 1)  # every pixel is a region of its own
    check(eng, split, NEW, 1, maxdiff, changed=split.size)
    joined = checkerboard(H, W, maxdiff)  # one region
    check(eng, joined, NEW, joined.size - 1, maxdiff, changed=0)
    check(eng, joined, NEW, joined.size, maxdiff, changed=joined.size)


def test_comb(eng):
    H, W = 64, 64
    img = comb(H, W, joined=True)
    n = region_size(img)
    check(eng, img, NEW, n - 1, 4, changed=0)
    check(eng, img, NEW, n, 4, changed=n)
    # at maxdiff 1 the joining row (242) holds the teeth of 241 .. 243 only
    got = check(eng, img, NEW, H, 1)
    assert 0 < int((got != img).sum()) < n
    teeth = comb(H, W, joined=False)
    lengths = sorted({H - 1 - x % 7 for x in range(0, W, 2)})
    assert len(lengths) == 7
    mid = lengths[3]  # the teeth of at most `mid` pixels go, the longer ones stay
    got = check(eng, teeth, NEW, mid, 4)
    assert 0 < int((got != teeth).sum()) < region_size(teeth)
    check(eng, teeth, NEW, lengths[-1], 4, changed=region_size(teeth))
    check(eng, teeth, NEW, lengths[0] - 1, 4, changed=0)


def test_ramp_connects_by_chain(eng):
    """Neighbours differ by maxdiff, the ends by thousands: connectivity is between neighbours,
    not relative to the pixel a region was seeded from."""
    H, W, maxdiff = 20, 130, 60
    img = np.broadcast_to((np.arange(W) * maxdiff - 3000).astype(np.int16), (H, W)).copy()
    assert int(img.max()) - int(img.min()) == (W - 1) * maxdiff > 7000
    check(eng, img, NEW, img.size - 1, maxdiff, changed=0)
    check(eng, img, NEW, img.size, maxdiff, changed=img.size)
    check(eng, img, NEW, H, maxdiff - 1, changed=img.size)  # columns of H pixels
    cut = img.copy()
    cut[:, 50:] += 1  # one step of maxdiff + 1: regions of 50 and 80 columns
    check(eng, cut, NEW, 50 * H, maxdiff, changed=50 * H)
    check(eng, cut, NEW, 50 * H - 1, maxdiff, changed=0)
    # a diagonal ramp: both neighbours of a pixel differ from it
    yy, xx = np.mgrid[:40, :45]
    diag = ((xx + yy) * maxdiff).astype(np.int16)
    check(eng, diag, NEW, diag.size - 1, maxdiff, changed=0)
    check(eng, diag, NEW, diag.size, maxdiff, changed=diag.size)
    check(eng, diag, NEW, 40, maxdiff - 1, changed=diag.size)  # anti-diagonals, 4-connected: single pixels


@pytest.mark.parametrize("maxsize", [1, 20, 255, 256, 257])
def test_exact_sizes(eng, maxsize):
    """count <= maxsize: a region of exactly maxsize pixels goes, one of maxsize + 1 stays; the
    two have the same value and only a column of newval between them."""
    w = 1 if maxsize < 20 else 5 if maxsize == 20 else 16
    h = maxsize // w  # maxsize = h * w + r
    r = maxsize - h * w
    img = np.full((h + 4, 2 * w + 3), NEW, np.int16)
    img[1:1 + h, 1:1 + w] = 96
    img[1 + h, 1:1 + r] = 96  # exactly maxsize
    img[1:1 + h, w + 2:2 * w + 2] = 96
    img[1 + h, w + 2:w + 3 + r] = 96  # maxsize + 1
    assert region_size(img) == 2 * maxsize + 1
    got = check(eng, img, NEW, maxsize, 0, changed=maxsize)
    assert (got[:, :w + 2] == NEW).all() and region_size(got) == maxsize + 1


def test_int16_extremes(eng):
    img = np.empty((8, 10), np.int16)
    img[:, :5], img[:, 5:] = -32768, 32767
    check(eng, img, 0, 40, 65535, changed=0)  # joined: one region of 80
    check(eng, img, 0, 40, 65534, changed=80)  # split: two of 40
    check(eng, img, 0, 80, 65535, changed=80)
    both = np.array([[-32768, 32767, -32768], [32767, -32768, 32767]], np.int16)
    check(eng, both, 0, 1, 65534, changed=6)
    check(eng, both, 0, 5, 65535, changed=0)
    # newval at an end of the range
    for newval in (-32768, 32767):  # the other half is one region of 40
        check(eng, img, newval, 39, 0, changed=0)
        check(eng, img, newval, 40, 0, changed=40)


@pytest.mark.parametrize("newval", [0, 80, NEW])
def test_newval_present_in_the_image(eng, newval):
    """Pixels that already hold newval are no region and separate the others."""
    img = blocky(60, 70, 8, newval=NEW, holes=0.05)
    assert (img == newval).any() and (img == 0).any() and (img == 80).any()
    for maxsize, maxdiff in ((6, 0), (30, 40), (400, 40)):
        got = check(eng, img, newval, maxsize, maxdiff)
    assert (got != img).any()


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2)])
def test_degenerate_shapes(eng, shape):
    rng = np.random.default_rng(shape[0] + 7 * shape[1])
    img = (np.repeat(rng.integers(0, 4, 120), 5)[:shape[0] * shape[1]] * 32).astype(np.int16).reshape(shape)
    img[rng.random(shape) < 0.1] = NEW
    assert np.array_equal(eng.filter_speckles(img, NEW, 0, 16), img)  # maxsize 0: unchanged
    for maxsize, maxdiff in ((1, 0), (4, 0), (5, 0), (9, 32), (300, 1000)):
        check(eng, img, NEW, maxsize, maxdiff)
    one = np.full(shape, 7, np.int16)
    check(eng, one, NEW, one.size, 0, changed=one.size)
    if one.size > 1:
        check(eng, one, NEW, one.size - 1, 0, changed=0)


def test_batch_of_different_images(eng):
    """nimg = 5 in one call: each image's result is its own, not its neighbour's."""
    import torch

    imgs = [serpentine(), uniform(64, 64), comb(), checkerboard(64, 64, 17), blocky(64, 64, 4)]
    assert len({i.shape for i in imgs}) == 1
    for maxsize, maxdiff in ((2000, 2), (2080, 17), (30, 0), (6, 0)):
        exps = [oracle(i, NEW, maxsize, maxdiff) for i in imgs]
        assert len({e.tobytes() for e in exps}) >= 3  # (two of them may both come out all newval)
        assert 2 <= sum(bool((e != i).any()) for e, i in zip(exps, imgs)) <= 4  # some change, some do not
        G = 64
        buf = torch.full((2 * G + 5 * 64 * 64,), 12345, dtype=torch.int16)
        buf[G:-G] = torch.from_numpy(np.stack(imgs).reshape(-1))
        buf = buf.cuda()
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.filter_speckles_device(buf.data_ptr() + 2 * G, 5, 64, 64, NEW, maxsize, maxdiff)
            eng.synchronize()
        finally:
            eng.set_stream(None)
        host = buf.cpu().numpy()
        assert (host[:G] == 12345).all() and (host[-G:] == 12345).all()
        got = host[G:-G].reshape(5, 64, 64)
        for k, (e, i) in enumerate(zip(exps, imgs)):
            assert np.array_equal(got[k], e), f"image {k}: {int((got[k] != e).sum())} px differ"
            assert np.array_equal(eng.filter_speckles(i, NEW, maxsize, maxdiff), e), k


def test_repeats(eng):
    """The order in which the links are made differs from run to run."""
    s, u = serpentine(), uniform()
    for _ in range(3):
        check(eng, s, NEW, region_size(s), 2, changed=region_size(s))
        check(eng, s, NEW, region_size(s) - 1, 2, changed=0)
        check(eng, u, NEW, u.size, 0, changed=u.size)
        check(eng, u, NEW, u.size - 1, 0, changed=0)
