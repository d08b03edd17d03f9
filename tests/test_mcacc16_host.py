"""McCnnAccurate's precision="bf16" without a device: the rounding ac_bf16 against
torch's, the CPU twin against exact numpy evaluations of dense integer scorers and against a numpy
restatement of its own float chain, the distance E_q between the two twins, argument errors, and
the default precision's bits."""
import numpy as np
import pytest

import mcacc16_cases as Q
import stereo_match_amd as sm
from stereo_match_amd import _lib


def check_bf16(x):
    """sm_mcacc_bf16_host against torch's float32 -> bfloat16 conversion on the CPU.  Values that
    are not NaN: bit for bit.  NaNs: torch's CPU conversion does not keep a NaN's sign (it gives one
    fixed pattern, 0x7FC0 or 0xFFFF by code path), so 'is NaN' is compared with torch, and the sign
    and the quiet bit with the input, which is what ac_bf16 promises."""
    import torch

    got = _lib.mcacc_bf16_host(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan_in = np.isnan(x)
    nan_want = ((want & 0x7F80) == 0x7F80) & ((want & 0x007F) != 0)
    nan_got = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
    assert np.array_equal(nan_want, nan_in) and np.array_equal(nan_got, nan_in)
    assert np.array_equal(got[~nan_in], want[~nan_in]), int((got[~nan_in] != want[~nan_in]).sum())
    bits = x.view(np.uint32)
    assert np.array_equal(got[nan_in] >> 15, (bits[nan_in] >> 31).astype(np.uint16))  # its sign
    assert ((got[nan_in] & 0x0040) != 0).all()  # quiet
    return int(nan_in.sum())


def test_bf16_rounding_every_upper_half():
    """All 65536 upper halves with the lower halves that decide: exact, one above, just below the
    tie, the tie (to even: both parities of the upper half occur), just above it, all ones; carries
    into the exponent, the overflow to infinity and subnormals are among them."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    nans = 0
    for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
        nans += check_bf16((hi | np.uint32(lo)).view(np.float32))
    assert nans > 0
    x = np.array([0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00008000, 0x00018000, 0x807F8000], np.uint32).view(np.float32)
    assert _lib.mcacc_bf16_host(x).tolist() == [0x7F80, 0x7F80, 0x7F7F, 0x0000, 0x0002, 0x8080]
    # the numpy restatement the integer evaluations use
    fin = (hi | np.uint32(0x8000)).view(np.float32)
    fin = fin[np.isfinite(fin) & (np.abs(fin) < 3e38)]
    assert np.array_equal(Q.bf16_round(fin).view(np.uint32) >> 16, _lib.mcacc_bf16_host(fin))


def test_bf16_rounding_random_bits():
    x = np.random.default_rng(5).integers(0, 2**32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert check_bf16(x) > 0


DENSE = [(2, 32, False), (3, 96, True), (4, 384, True), (2, 384, False)]


@pytest.mark.parametrize("F,U,bites", DENSE)
def test_dense_integer_scorer(F, U, bites):
    """The raw bf16 twin equals the exact evaluation with explicit rounding, value for value, in
    both roles.  With three or more layers the activations leave bf16's exact range: the rounding
    changes some, exact ties are among them, and the f32 twin gives other values."""
    m = Q.dense_model(F, U)
    assert m.precision == "bf16"
    fa, fb = Q.int_features("tiny", 0), Q.int_features("tiny", 1)
    for left in (True, False):
        want, info = Q.int_volume16(F, U, "tiny", 20, 0, left)
        print(F, U, left, info)
        assert 0 < info["peak"] < 2**24
        if F >= 3:
            assert bites and max(info["changed"]) > 0 and info["ties"] > 0
        else:
            assert not bites and max(info["changed"]) == 0
        got = m.join(fa, fb, 20, 0, a_is_left=left, raw=True, host=True)
        assert got.shape == (1,) + want.shape and Q.same_bits(got[0], want), int((got[0] != want).sum())
        f32 = m.with_precision("f32").join(fa, fb, 20, 0, a_is_left=left, raw=True, host=True)
        if bites:
            assert not Q.same_bits(f32[0], want)
            if (F, U) == (4, 384):
                assert (f32[0] != want)[~np.isnan(want)].mean() > 0.5
        else:
            assert Q.same_bits(f32[0], want)
        # the sigmoid of those values, and the roles differ
        s = m.join(fa, fb, 20, 0, a_is_left=left, host=True)
        ok = ~np.isnan(want)
        assert np.array_equal(s[0][ok], -_lib.mcacc_sigmoid_host(-want[ok]))
    assert not Q.same_bits(Q.int_volume16(F, U, "tiny", 20, 0, True)[0], Q.int_volume16(F, U, "tiny", 20, 0, False)[0])


def check_sweep_conditions(F, info):
    """What makes a case of the width sweep (here and in test_gpu_mcacc_widths.py) say something:
    every sum exact in float32, and with three or more layers operands the rounding changes, exact
    ties among them.  With two layers the hidden operands are below 2^8 and nothing is rounded."""
    assert 0 < info["peak"] < 2**24
    if F >= 3:
        assert max(info["changed"]) > 0 and info["ties"] > 0
    else:
        assert max(info["changed"]) == 0


@pytest.mark.parametrize("U", Q.UNITS)
@pytest.mark.parametrize("F", [2, 3, 4])
def test_dense_integer_scorer_every_width(F, U):
    """Every hidden width the scorer takes, on the 11 x 37 map with 6 planes from offset 1 (ragged
    against the device's 32-column and 4-plane tiles): the raw bf16 twin equals the exact evaluation
    in both roles."""
    m = Q.dense_model(F, U)
    fa, fb = Q.int_features("odd", 0), Q.int_features("odd", 1)
    for left in (True, False):
        want, info = Q.int_volume16(F, U, "odd", 6, 1, left)
        check_sweep_conditions(F, info)
        got = m.join(fa, fb, 6, 1, a_is_left=left, raw=True, host=True)
        assert got.shape == (1,) + want.shape and Q.same_bits(got[0], want), int((got[0] != want).sum())
    assert not Q.same_bits(Q.int_volume16(F, U, "odd", 6, 1, True)[0], Q.int_volume16(F, U, "odd", 6, 1, False)[0])


def test_width_sweep_figures():
    """The figures DESIGN.md §4.21 states for the sweep: the largest sum of magnitudes, and the
    smallest share of a layer's operands the rounding changes at three or more layers."""
    peaks, least = {}, 1.0
    for F in (2, 3, 4):
        for U in Q.UNITS:
            for left in (True, False):
                info = Q.int_volume16(F, U, "odd", 6, 1, left)[1]
                peaks[F, U] = max(peaks.get((F, U), 0), info["peak"])
                if F >= 3:
                    least = min(least, max(info["changed"]))
    top = max(peaks, key=peaks.get)
    print(f"width sweep: largest peak {peaks[top]} at {top}, least changed share {least:.4f}")
    assert top == (4, 352) and peaks[top] == 4544944  # the left role's; the right role's is 4301246
    assert least >= 0.012


def test_tall_integer_scorer():
    """65538 rows of 2 columns, more rows than a grid has workgroup rows: the twins equal the exact
    evaluation there, bf16 and (nothing being rounded at two layers) f32."""
    fa, fb = Q.int_features("tall", 0), Q.int_features("tall", 1)
    want, info = Q.int_volume16(2, 32, "tall", 2, 0)
    check_sweep_conditions(2, info)
    assert np.isnan(want[1, :, 0]).all() and np.isfinite(want[0]).all() and np.isfinite(want[1, :, 1]).all()
    for precision in ("bf16", "f32"):
        got = Q.dense_model(2, 32, precision).join(fa, fb, 2, 0, raw=True, host=True)
        assert Q.same_bits(got[0], want)


@pytest.mark.parametrize("F,U", [(1, 32), (2, 96), (4, 64)])
def test_twin_is_its_chain(F, U):
    """Random float hidden layers: the twin equals sequential float32 additions of the exact
    products in ascending k, bit for bit, in both roles and with an offset."""
    m = Q.exact_head_net(F, U)
    fa, fb = Q.int_features("narrow", 0), Q.int_features("narrow", 1)
    for left in (True, False):
        want = Q.chain_volume16(m, fa, fb, 7, -2, left)
        got = m.join(fa, fb, 7, -2, a_is_left=left, raw=True, host=True)
        assert Q.same_bits(got[0], want), int((got[0] != want).sum())
    if F > 1:
        f32 = m.with_precision("f32").join(fa, fb, 7, -2, raw=True, host=True)
        assert not Q.same_bits(f32[0], Q.chain_volume16(m, fa, fb, 7, -2, True))


@pytest.mark.parametrize("name,D,m0", [("tiny", 20, 0), ("ragged", 12, -3)])
@pytest.mark.parametrize("F,U", [(2, 96), (3, 384), (4, 384)])
def test_rounding_moves_random_nets(name, D, m0, F, U):
    """E_q = max |twin_bf16 - twin_f32| of the raw volume: above zero (the mode does something) and
    small against the values."""
    eq = Q.e_q(name, D, m0, F, U)
    scale = float(np.nanmax(np.abs(Q.twin_raw(name, D, m0, F, U, "f32"))))
    print(f"E_q {name} D={D} m={m0} F={F} U={U}: {eq:.3e} (largest |z| {scale:.3e})")
    assert 0 < eq < 0.1 * scale


def test_f1_has_no_hidden_layer():
    """F = 1 is accepted and its bf16 twin is the f32 twin: nothing is rounded."""
    m = Q.float_net(1, 32)
    fa, fb = Q.twin_features("tiny", 2, 0), Q.twin_features("tiny", 2, 1)
    assert Q.same_bits(m.join(fa, fb, 20, 0, host=True), m.with_precision("f32").join(fa, fb, 20, 0, host=True))


def test_arguments_and_default():
    base = Q.model(2, 3, 96)
    assert base.precision == "f32" and sm.McCnnAccurate.random(1, 1, 32).precision == "f32"
    with pytest.raises(AttributeError):
        base.precision = "bf16"
    for bad in ("fp16", "BF16", None, 1):
        with pytest.raises(ValueError, match="precision"):
            sm.McCnnAccurate.random(1, 1, 32, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            base.with_precision(bad)
        with pytest.raises(ValueError, match="precision"):
            sm.McCnnAccurate(base.weights, base.biases, base.fc_weights, base.fc_biases, precision=bad)
    q = base.with_precision("bf16")
    assert q.precision == "bf16" and base.precision == "f32" and q is not base
    for mine, theirs in zip(q.weights + q.biases + q.fc_weights + q.fc_biases,
                            base.weights + base.biases + base.fc_weights + base.fc_biases):
        assert mine is theirs and not mine.flags.writeable
    assert q.with_precision("f32").precision == "f32"
    assert (q.layers, q.fc_layers, q.units, q.device) == (base.layers, base.fc_layers, base.units, base.device)
    # precision="f32" is the net built without the argument
    fa, fb = Q.twin_features("tiny", 2, 0), Q.twin_features("tiny", 2, 1)
    explicit = sm.McCnnAccurate(base.weights, base.biases, base.fc_weights, base.fc_biases, precision="f32")
    want = base.join(fa, fb, 9, -2, host=True)
    assert Q.same_bits(explicit.join(fa, fb, 9, -2, host=True), want)
    assert Q.same_bits(q.with_precision("f32").join(fa, fb, 9, -2, host=True), want)
    assert not Q.same_bits(q.join(fa, fb, 9, -2, host=True), want)
    assert sm.McCnnAccurate.random(2, 2, 64, seed=3, precision="bf16").precision == "bf16"


def test_from_npz_takes_precision(tmp_path):
    base = Q.model(1, 2, 32)
    path = str(tmp_path / "net.npz")
    base.save_npz(path)
    assert sm.McCnnAccurate.from_npz(path).precision == "f32"
    q = sm.McCnnAccurate.from_npz(path, precision="bf16")
    assert q.precision == "bf16" and np.array_equal(q.fc_weights[1], base.fc_weights[1])
    with pytest.raises(ValueError, match="precision"):
        sm.McCnnAccurate.from_npz(path, precision="half")


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan, 3.4e38, -3.4e38])
def test_hidden_weight_bf16_cannot_hold(value):
    """A hidden-layer weight that is not finite or rounds to infinity: an error in bf16 mode only;
    the first and the last layer stay f32 and may hold it."""
    base = Q.model(1, 3, 32)
    fws = [np.array(w) for w in base.fc_weights]
    fws[2][5, 7] = value
    ok = sm.McCnnAccurate(base.weights, base.biases, fws, base.fc_biases)  # f32 accepts what it accepted
    with pytest.raises(ValueError, match="scorer layer 2"):
        ok.with_precision("bf16")
    with pytest.raises(ValueError, match="scorer layer 2"):
        sm.McCnnAccurate(base.weights, base.biases, fws, base.fc_biases, precision="bf16")
    fa = Q.twin_features("tiny", 1, 0)
    vol = np.empty((1, 2) + fa.shape[:2], np.float32)
    args = (3, 32, _lib._ptr_array(fws), _lib._ptr_array(list(base.fc_biases)), fa.ctypes.data, fa.ctypes.data, 1,
            fa.shape[0], fa.shape[1], 2, 0, 1, 1, vol.ctypes.data)
    assert _lib.load().sm_mcacc_join_host_bf16(*args) == _lib.SM_E_ARG
    assert _lib.load().sm_mcacc_join_host(*args) == _lib.SM_OK
    if abs(value) == 3.4e38:  # finite and below bf16's overflow threshold elsewhere: only hidden layers are rounded
        fws = [np.array(w) for w in base.fc_weights]
        fws[0][5, 7] = value
        fws[3][0, 7] = value
        assert sm.McCnnAccurate(base.weights, base.biases, fws, base.fc_biases, precision="bf16").precision == "bf16"
    fws = [np.array(w) for w in base.fc_weights]
    fws[1][0, 0] = np.float32(3.38e38)  # rounds to bf16's largest finite value's neighbourhood, not to infinity
    assert sm.McCnnAccurate(base.weights, base.biases, fws, base.fc_biases, precision="bf16").precision == "bf16"
