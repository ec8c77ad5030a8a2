"""GPU: the fitted noise floor (pplib.get_noise_fit, pplib.py:2341-2373, and
the find_kc it calls, pplib.py:1530-1561) against the reference's values in
tests/golden/noisefit.npz (make_golden_noisefit.py): kc equal, noise within
the rtol 1e-12 get_noise_PS is held to (test_gpu_parity.py,
test_gpu_fftplans.py: the tail mean is the same sum).  kc parity is defined
because every stored winner leads the other a indices by more than a
relative 1e-6 in chi-squared (test_noisefit_host.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "noisefit.npz"))
PULSE = [str(c) for c in G["cases"]]
EDGE = ["edge_4095", "edge_8192"]     # past 48 KB of LDS per workgroup
LONG = ["port_8x2048", "port_9x1000"]
FACT = float(G["fact"])
RTOL = 1e-12


def _np(t):
    return t.cpu().numpy()


def _case(name, dtype):
    """(rows of dtype as the device gets them, reference noise, kc).  The
    float32 expectation is the reference on the float32-rounded rows; the
    cases stored as float32 alone serve both."""
    sfx = "__f32" if dtype == np.float32 and name + "__rows__f32" in G else ""
    rows = G[name + "__rows" + sfx].astype(dtype)
    if name in LONG:
        rows = rows.reshape(1, -1)           # chans=False: the ravelled portrait
    return rows, G[name + "__noise" + sfx], G[name + "__kc" + sfx]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", PULSE + ["clamp_64"] + EDGE + LONG)
def test_noise_fit_matches_the_reference(name, dtype):
    """Every stored case, float32 and float64 input, twice (bitwise equal)."""
    from pulseportraiture_amd import engine
    rows, want, kc = _case(name, dtype)
    noise, got_kc = engine.noise_fit_rows(rows, FACT)
    noise, got_kc = _np(noise), _np(got_kc)
    print("NOISEFIT %s %s: kc %s (reference %s), noise max rel dev %.1e" %
          (name, np.dtype(dtype).name, got_kc, kc,
           np.abs(noise / want - 1).max()))
    assert got_kc.dtype == np.int32 and noise.dtype == np.float64
    np.testing.assert_array_equal(got_kc, kc)
    np.testing.assert_allclose(noise, want, rtol=RTOL)
    again = engine.noise_fit_rows(rows, FACT)
    np.testing.assert_array_equal(_np(again[0]), noise)
    np.testing.assert_array_equal(_np(again[1]), got_kc)
    # which entry served it
    assert engine._noise_batch_len_ok(rows.shape[-1]) == (name not in LONG)


def test_get_noise_method_fit():
    """The public entry points: pplib.get_noise(method="fit") on a profile,
    per channel and on a whole portrait (chans=False ravels it: a long
    row)."""
    from pulseportraiture_amd import pplib
    rows, want, _ = _case("pulse_256", np.float64)
    got = pplib.get_noise(rows[0], method="fit")
    assert isinstance(got, np.float64)
    np.testing.assert_allclose(got, want[0], rtol=RTOL)
    rows, want, _ = _case("pulse_2048", np.float64)
    got = pplib.get_noise(rows, method="fit", chans=True)
    assert got.shape == (3,) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=RTOL)
    np.testing.assert_allclose(pplib.get_noise_fit(rows, FACT, True), want,
                               rtol=RTOL)
    rows, want, _ = _case("pulse_1001", np.float32)
    np.testing.assert_allclose(pplib.get_noise(rows, "fit", chans=True), want,
                               rtol=RTOL)
    for name in LONG:
        port = G[name + "__rows"]
        np.testing.assert_allclose(pplib.get_noise(port, method="fit"),
                                   G[name + "__noise"][0], rtol=RTOL)
    assert pplib.default_noise_method == "PS"


def test_find_kc():
    """pplib.find_kc on stored power spectra: both fns, scalar and array
    errs; an int; 0 for an unknown fn."""
    from pulseportraiture_amd import engine, pplib
    for name in PULSE + EDGE + LONG:
        for p, kc in zip(G[name + "__pows"], G[name + "__kc"]):
            got = pplib.find_kc(p)
            assert type(got) is int and got == kc, (name, got, kc)
    p = G["pulse_256__pows"][0]
    errs = G["half_tri__errs_array"]
    assert pplib.find_kc(p, errs) == G["exp_dc__kc_array"]
    assert pplib.find_kc(p, 0.5, "exp_dc") == G["pulse_256__kc"][0]
    for key in ("scalar", "array"):
        got = pplib.find_kc(G["half_tri__pows_" + key],
                            G["half_tri__errs_" + key], fn="half_tri")
        assert type(got) is int and got == G["half_tri__kc_" + key], key
    assert pplib.find_kc(p, fn="gaussian") == 0
    # a batch of spectra in one launch, and again
    kc = _np(engine.find_kc_rows(G["pulse_2048__pows"]))
    np.testing.assert_array_equal(kc, G["pulse_2048__kc"])
    np.testing.assert_array_equal(
        _np(engine.find_kc_rows(G["pulse_2048__pows"])), kc)
    with pytest.raises(ValueError):
        engine.find_kc_rows(p, errs[:5])


def test_degenerate_rows_end_alone():
    """An all-zero row and a row holding NaNs return what the reference
    returned for them (log10 0 and NaN make brute's whole grid NaN: index 0,
    kc = N - 1, the clamp; noise 0 and NaN), and the clean rows beside them
    are bitwise those of a launch without them -- in LDS and from spectra."""
    from pulseportraiture_amd import engine
    rows = G["degenerate__rows"]
    assert (rows[1] == 0).all() and np.isnan(rows[2]).sum() == 2
    noise, kc = (_np(t) for t in engine.noise_fit_rows(rows, FACT))
    print("NOISEFIT degenerate: kc %s noise %s" % (kc, noise))
    np.testing.assert_array_equal(kc, G["degenerate__kc"])
    want = G["degenerate__noise"]
    assert want[1] == 0.0 and np.isnan(want[2])
    assert noise[1] == 0.0 and np.isnan(noise[2])
    np.testing.assert_allclose(noise[[0, 3]], want[[0, 3]], rtol=RTOL)
    clean = engine.noise_fit_rows(rows[[0, 3]], FACT)
    np.testing.assert_array_equal(_np(clean[0]), noise[[0, 3]])
    np.testing.assert_array_equal(_np(clean[1]), kc[[0, 3]])
    pows = G["degenerate__pows"]
    with np.errstate(all="ignore"):
        kcs = _np(engine.find_kc_rows(pows))
    np.testing.assert_array_equal(kcs, G["degenerate__kc"])
    np.testing.assert_array_equal(_np(engine.find_kc_rows(pows[[0, 3]])),
                                  kcs[[0, 3]])


def test_unsupported_lengths_are_refused():
    """nbin 30 through the batch entry is PPF_EUNSUP; a row past
    ppf_noise_long's limit has no workspace."""
    import torch
    from pulseportraiture_amd import _lib, engine
    dev = engine.device()
    lib, ctx = _lib.load(), _lib.context(dev.index)
    x = torch.zeros((2, 30), dtype=torch.float64, device=dev)
    noise = torch.empty(2, dtype=torch.float64, device=dev)
    kc = torch.empty(2, dtype=torch.int32, device=dev)
    a, t = engine.find_kc_tables(16)
    rc = lib.ppf_noise_fit_batch(ctx, 2, 30, _lib.PPF_F64, engine._p(x), FACT,
                                 a.ctypes.data, t.ctypes.data,
                                 engine._p(noise), engine._p(kc), None)
    assert rc == _lib.PPF_EUNSUP
    with pytest.raises(NotImplementedError):
        _lib.check(rc, ctx)
    n = (1 << 25) + 2
    assert lib.ppf_noise_fit_long_workspace_bytes(1, n) == 0
    big = torch.empty((1, n), dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError):
        engine.noise_fit_rows(big, FACT)
    # the dispatcher sends a 30-sample row to the long entry, which takes it
    got = engine.noise_fit_rows(np.arange(30.0)[None, :] ** 2 % 7, FACT)
    assert np.isfinite(_np(got[0])).all()
