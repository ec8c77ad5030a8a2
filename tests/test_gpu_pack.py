"""ppf_pack_psrfits_batch (k_pack_wave, k_pack_block, k_pack_f32) through
engine.pack_rows: 16-bit packing is psrfits.quantize bit for bit (bytes,
DAT_SCL, DAT_OFFS), float32 packing is astype('>f4'), both are reproducible,
and a file written from device rows reads back through the unpack kernel
within the quantisation step.

Shapes: every nbin of {1, 2, 7, 8, 63, 64, 65, 256, 257, 1025, 8200} and every
nrow of {1, 3, 65, 1000}, the row lengths without 16-byte aligned rows at
nrow > 1; both sides of the wave-per-row / workgroup-per-row switch (2048 |
2049, the latter with and without aligned rows); and row counts past one
launch's grid, where a workgroup strides (wave kernel: 4 x 8192 rows; block
and float32 kernels: 8192 workgroups)."""
import numpy as np
import pytest

from pulseportraiture_amd import psrfits

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)

SHAPES = [(3, 1), (65, 2), (1000, 7), (1, 8), (65, 63), (1000, 64), (3, 65),
          (65, 256), (3, 257), (3, 1025), (1, 8200), (3, 8200),
          (5, 2048), (3, 2049), (3, 2056)]
# grid-stride: (rows, bins, dtype) once each
LONG = [(33000, 9, np.float64), (33000, 8, np.float32),
        (8500, 2049, np.float32)]


def _rows(nrow, nbin, dtype, seed=0):
    rng = np.random.default_rng(1000 * nbin + nrow + seed)
    x = rng.normal(size=(nrow, nbin)) * rng.uniform(0.1, 50.0, (nrow, 1)) + \
        rng.normal(size=(nrow, 1)) * 20.0
    return x.astype(dtype)


def _pack(x, elem="I"):
    import torch
    from pulseportraiture_amd import engine
    raw, scl, offs = engine.pack_rows(x, elem=elem)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), scl.cpu().numpy(), offs.cpu().numpy()


def _quantize(x):
    """psrfits.quantize of rows [nrow, nbin]: (file bytes, scl, offs)."""
    q, scl, offs = psrfits.quantize(np.asarray(x)[None, None])
    return q[0, 0].astype(">i2").view(np.uint8), scl[0], offs[0]


def _assert_quantized(x, got):
    raw, scl, offs = got
    wraw, wscl, woffs = _quantize(x)
    assert raw.dtype == np.uint8 and raw.shape == wraw.shape
    assert scl.dtype == np.float32 and offs.dtype == np.float32
    np.testing.assert_array_equal(scl.view(np.uint32), wscl.view(np.uint32))
    np.testing.assert_array_equal(offs.view(np.uint32), woffs.view(np.uint32))
    np.testing.assert_array_equal(raw, wraw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nrow,nbin", SHAPES)
def test_int16_packing_is_quantize_bit_for_bit(nrow, nbin, dtype):
    x = _rows(nrow, nbin, dtype)
    _assert_quantized(x, _pack(x))


@pytest.mark.parametrize("nrow,nbin,dtype", LONG)
def test_int16_packing_past_one_grid(nrow, nbin, dtype):
    x = _rows(nrow, nbin, dtype)
    _assert_quantized(x, _pack(x))


@pytest.mark.parametrize("nbin", [16, 13])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_directed_rows(nbin, dtype):
    rng = np.random.default_rng(nbin)
    const = np.full(nbin, 3.25)
    ends = rng.uniform(-1.0, 1.0, nbin)
    ends[0], ends[-1] = -7.5, 9.25               # min first, max last
    neg = -rng.uniform(1.0, 100.0, nbin)
    wide = 10.0 ** rng.uniform(-3.0, 9.0, nbin)
    wide[3], wide[5] = 1e-3, 1e9
    tie = rng.integers(-1000, 1000, nbin).astype(float)
    tie[0], tie[-1] = -32767.0, 32767.0          # offs 0, scl 1
    tie[1:5] = [0.5, 1.5, 2.5, -0.5]
    x = np.stack([const, ends, neg, wide, tie]).astype(dtype)
    raw, scl, offs = got = _pack(x)
    _assert_quantized(x, got)
    q = raw.view(">i2")
    # the constant row: the 1e-30 floor, every sample 0
    assert scl[0] == np.float32(1e-30) and offs[0] == np.float32(3.25)
    assert (q[0] == 0).all()
    assert q[1, 0] == -32767 and q[1, -1] == 32767
    assert offs[2] < 0 and q[2].min() == -32767 and q[2].max() == 32767
    assert q[3, 5] == 32767 and q[3, 3] == -32767
    # ties round half to even
    assert scl[4] == 1.0 and offs[4] == 0.0
    np.testing.assert_array_equal(q[4, 1:5], [0, 2, 2, 0])
    np.testing.assert_array_equal(q[4, 5:-1], tie[5:-1])


E_SHAPES = [(nrow, nbin, dt) for nrow, nbin in
            [(1, 8), (3, 7), (65, 64), (3, 1025), (1000, 5), (3, 1)]
            for dt in (np.float32, np.float64)] + [(33000, 257, np.float32)]


@pytest.mark.parametrize("nrow,nbin,dtype", E_SHAPES)
def test_float32_packing(nrow, nbin, dtype):
    x = _rows(nrow, nbin, dtype)
    if dtype == np.float64:
        x[0, 0] = 1e-50                # rounds to 0 in float32
    raw, scl, offs = _pack(x, "E")
    assert raw.shape == (nrow, nbin * 4) and raw.dtype == np.uint8
    np.testing.assert_array_equal(raw,
                                  x.astype(">f4").view(np.uint8))
    assert (scl == 1.0).all() and (offs == 0.0).all()
    assert scl.shape == offs.shape == (nrow,)


@pytest.mark.parametrize("elem", ["I", "E"])
def test_two_calls_give_identical_bytes(elem):
    x = _rows(65, 257, np.float64)
    a, b = _pack(x, elem), _pack(x, elem)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint8), v.view(np.uint8))


def test_leading_shape_and_tensor_input():
    import torch
    from pulseportraiture_amd import engine
    x = _rows(24, 16, np.float64).reshape(2, 3, 4, 16)
    got = _pack(x)
    _assert_quantized(x.reshape(24, 16), got)
    t = torch.from_numpy(x).cuda()
    for a, b in zip(got, _pack(t)):
        np.testing.assert_array_equal(a, b)
    # an unaligned base pointer takes the element-wide path: same bytes
    flat = torch.zeros(24 * 16 + 1, dtype=torch.float64, device="cuda")
    flat[1:] = t.reshape(-1)
    for a, b in zip(got, _pack(flat[1:].reshape(24, 16))):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        engine.pack_rows(x, elem="B")


def _unpacked(filename):
    import torch
    from pulseportraiture_amd import engine
    f = psrfits.PSRFITS(filename)
    raw, edt = f.data_bytes()
    scl, offs = f.scales_offsets()
    elem = {np.dtype(">i2"): 0, np.dtype(">f4"): 2}[edt]
    out = engine.unpack_psrfits(torch.from_numpy(np.array(raw)).cuda(), elem,
                                f.npol, f.nchan, f.nbin, scl, offs,
                                rm_baseline=False)
    torch.cuda.synchronize()
    shape = (f.nsub, f.npol, f.nchan, f.nbin)
    wts = f.weights()
    f.close()
    return out["rows"].cpu().numpy(), scl, offs, shape, wts


@pytest.mark.parametrize("device_input", [False, True])
def test_round_trip_through_a_file(tmp_path, device_input):
    """write_archive_rows -> PSRFITS -> k_unpack: per sample
    |x' - x| <= 0.5 scl + 2 eps32 (|offs| + 32768 scl), the quantisation
    half-step plus the float32 arithmetic of the unpack."""
    nsub, nchan, nbin = 2, 5, 64
    rng = np.random.default_rng(11)
    x = rng.normal(size=(nsub, 1, nchan, nbin)) * \
        rng.uniform(0.5, 30.0, (nsub, 1, nchan, 1))
    x[:, :, 1] += 1e4                  # a large pedestal on a small range
    x[:, :, 2] = 0.75                  # a constant profile
    data = x
    if device_input:
        import torch
        data = torch.from_numpy(x).cuda()
    name = str(tmp_path / "rt.fits")
    freqs = np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1))
    wts = np.ones((nsub, nchan))
    wts[1, 3] = 0.0
    psrfits.write_archive_rows(name, data, freqs, wts, np.full(nsub, 0.004),
                               np.array([5.0, 15.0]), np.full(nsub, 10.0))
    rows, scl, offs, shape, wts_f = _unpacked(name)
    assert shape == (nsub, 1, nchan, nbin)
    np.testing.assert_array_equal(wts_f, wts)
    _, wscl, woffs = psrfits.quantize(x)
    np.testing.assert_array_equal(scl, wscl)
    np.testing.assert_array_equal(offs, woffs)
    s = scl.reshape(nsub, nchan, 1).astype(np.float64)
    o = offs.reshape(nsub, nchan, 1).astype(np.float64)
    bound = 0.5 * s + 2 * EPS32 * (np.abs(o) + 32768 * s)
    err = np.abs(rows.astype(np.float64) - x[:, 0])
    print("round trip: max err / bound = %.3f" % (err / bound).max())
    assert (err <= bound).all()
    # float32 samples come back as the float32 values of the rows
    psrfits.write_archive_rows(name, data, freqs, wts, np.full(nsub, 0.004),
                               np.array([5.0, 15.0]), np.full(nsub, 10.0),
                               elem="E")
    rows, scl, offs, shape, _ = _unpacked(name)
    assert (scl == 1.0).all() and (offs == 0.0).all()
    np.testing.assert_array_equal(rows, x[:, 0].astype(np.float32))
