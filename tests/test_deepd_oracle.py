"""CPU: the oracle's own maps of the numDisparities 272..512 cases (tests/deepd_cases.py) reach the
planes the GPU tests are there for.  A GPU comparison against a map with no winner above plane
256 would pass on any kernel that gets planes 0..255 right, so every case must have at least
MIN_VALID of the frame valid and MIN_DEEP of the valid pixels on planes >= 256."""
import numpy as np
import pytest

import deepd_cases as C
from oracle import sgm_np


@pytest.mark.parametrize("D,minD,kind", C.IMAGE_CASES, ids=[f"D{d}_minD{m}_{k}" for d, m, k in C.IMAGE_CASES])
def test_image_case_reaches_the_deep_planes(D, minD, kind):
    disp, wta = C.expected_wta(D, minD, kind)
    valid, deep = C.coverage(disp, minD)
    print(f"D {D} minD {minD} {kind}: valid {valid:.3f}, on planes >= 256 {deep:.3f}")
    assert valid >= C.MIN_VALID
    assert deep >= C.MIN_DEEP
    assert int(wta.max()) >= 256 and int(wta.max()) < D


@pytest.mark.parametrize("Dv,shifts", C.VOLUME_CASES, ids=[f"Dv{d}" for d, _ in C.VOLUME_CASES])
def test_volume_case_reaches_the_deep_planes(Dv, shifts):
    disp = C.expected_volume(Dv, shifts)
    valid, deep = C.coverage(disp, 0)
    print(f"Dv {Dv}: valid {valid:.3f}, on planes >= 256 {deep:.3f}")
    assert valid >= C.MIN_VALID
    assert deep >= C.MIN_DEEP


def test_numpy_and_c_oracles_agree_at_272():
    a, b = C.image_pair(272, 0)
    for kind in ("census8", "sgbm5"):
        p = C.params(kind, 272)
        assert np.array_equal(sgm_np.compute(a, b, p), C.expected(272, 0, kind))
