"""fastNlMeansDenoising: known answers of the numpy restatement (tests/nlm_np.py, DESIGN.md
§4.8).  CPU only: the package's own table (sm_nlm_weight_table) and kernel are checked against
the same restatement in tests/test_gpu_nlm.py."""
import os

import numpy as np
import pytest

import nlm_np

GOLDEN_NLM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlm",
                          "nlm_h10_t7_s21_40x56.npz")

# (h, tws, sws): fpm, shift, n, last non-zero index (None: not recorded)
TABLE_KATS = [
    ((10, 7, 21), 19096, 6, 49785, 527),
    ((3, 7, 21), 19096, 6, 49785, 47),
    ((30, 7, 21), 19096, 6, 49785, 4745),
    ((10, 5, 11), 69599, 5, 50801, 539),
    ((10, 3, 5), 336860, 4, 36577, 388),
    ((4, 8, 22), 15919, 7, 41149, 70),  # even sizes count as 9 and 23
]


@pytest.mark.parametrize("prm,fpm,shift,n,last", TABLE_KATS, ids=[str(k[0]) for k in TABLE_KATS])
def test_table_kats(prm, fpm, shift, n, last):
    tab, f, s = nlm_np.weight_table(*prm)
    assert (f, s, len(tab)) == (fpm, shift, n)
    assert tab[0] == fpm
    assert int(np.nonzero(tab)[0][-1]) == last
    assert np.all(np.diff(tab) <= 0), "the table must be non-increasing"
    assert tab[last] >= 0.001 * fpm


def test_table_h10_values():
    tab, _, _ = nlm_np.weight_table(10, 7, 21)
    assert (tab[0], tab[1], tab[527], tab[528]) == (19096, 18848, 20, 0)


def test_table_even_sizes_are_the_next_odd():
    a = nlm_np.weight_table(4, 8, 22)
    b = nlm_np.weight_table(4, 9, 23)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert nlm_np.windows(8, 22) == (4, 9, 11, 23, 15)


def test_table_h0():
    tab, fpm, _ = nlm_np.weight_table(0, 7, 21)
    assert tab[0] == fpm and not tab[1:].any()
    assert np.all(np.diff(tab) <= 0)


def test_constant_image():
    img = np.full((11, 17), 93, np.uint8)
    out, wsum = nlm_np.denoise(img, 10, 7, 21)
    assert np.array_equal(out, img)
    assert np.all(wsum == 21 * 21 * 19096)


def test_one_pixel():
    img = np.array([[201]], np.uint8)
    for fn in (nlm_np.denoise, nlm_np.denoise_direct):
        out, wsum = fn(img, 10, 7, 21)
        assert np.array_equal(out, img)
        assert wsum[0, 0] == 21 * 21 * 19096  # every offset reads the only sample


def test_random_bytes_denoise_to_themselves():
    """Independent uniform bytes: every non-centre patch distance is past the table's non-zero
    prefix at (10, 7, 21), so only the centre offset has weight (seed 0 is one where it holds)."""
    img = np.random.default_rng(0).integers(0, 256, (30, 45), dtype=np.uint8)
    out, wsum = nlm_np.denoise(img, 10, 7, 21)
    assert np.array_equal(out, img)
    assert np.all(wsum == 19096)


@pytest.mark.parametrize("shape", [(9, 13), (3, 2)])
@pytest.mark.parametrize("prm", [(10, 7, 21), (30, 5, 11), (10, 4, 6)])
def test_direct_equals_vectorised(shape, prm):
    img = nlm_np.noisy_blobs(*shape, seed=3)
    a = nlm_np.denoise(img, *prm)
    b = nlm_np.denoise_direct(img, *prm)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[0] != img).any(), "the case must not degenerate to the identity"


def test_reflect101_border():
    row = np.arange(4, dtype=np.uint8)[None, :]
    e = nlm_np.extend(row, 7)
    # period 2 * (4 - 1) = 6 along x, reflected more than once; the length-1 axis repeats
    assert e.shape == (15, 18)
    assert e[0].tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert np.all(e == e[0])


def test_golden_fixture_reproduces():
    z = np.load(GOLDEN_NLM, allow_pickle=False)
    h, tws, sws = (int(v) for v in z["params"])
    assert (h, tws, sws) == (10, 7, 21) and z["src"].shape == (40, 56)
    out, wsum = nlm_np.denoise(z["src"], h, tws, sws)
    assert np.array_equal(out, z["out"])
    assert np.array_equal(wsum, z["wsum"])
    # the regime the GPU tests want: many offsets carry weight
    assert np.median(z["wsum"]) > 4 * 19096
    assert (z["out"] != z["src"]).mean() > 0.5
