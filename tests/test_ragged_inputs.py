"""Host checks of the ragged-channel cases (tests/ragged.py): the inputs
have the properties tests/test_gpu_ragged.py relies on to reach each kernel
path, and every fit is well posed, so that a device deviation there is the
device's.  No GPU."""
import numpy as np
import pytest

import goldens as G
import ragged as R

# the cases of the issue's table: none may go missing
EXPECTED = {
    "w2_guess": {(2048, 33), (2048, 100), (2048, 250)},
    "w2_dsum": {(2048, 100), (2048, 250)},
    "xmom": {(256, 250), (512, 37), (1024, 100), (2048, 161)},
    "momx": {(512, 100)},
    "pass": {(512, 97), (2048, 100)},
    "warm": {(256, 257), (256, 513)},
    "wm": {(1000, 45), (1536, 100)},
    "wo": {(1001, 33), (1001, 37)},
    "blk": {(512, 3), (512, 17), (512, 31), (4096, 45), (128, 45)},
    "long": {(8194, 5)},
    "swz": {(256, 256), (100, 256), (35, 256), (64, 256), (2050, 256)},
}


def test_case_table_is_complete():
    got = {}
    for c in R.CASES:
        got.setdefault(c["family"], set()).add((c["nbin"], c["nchan"]))
    assert got == EXPECTED
    assert len(set(R.CASE_NAMES)) == len(R.CASES)
    by = {n: R.case(n) for n in R.CASE_NAMES}
    # both data types on the guess path, GM once on the fused pass, all five
    # parameters at 2048 bins, tau at 17 channels, both fits at odd nbin
    for n in (33, 100, 250):
        for dt in ("f32", "f64"):
            assert "w2_guess-%dx2048-pd-cut-%s" % (n, dt) in by
    assert any(c["family"] == "xmom" and c["flags"] == R.PDG for c in R.CASES)
    assert by["pass-100x2048-pdgta-cut-f32"]["flags"] == R.ALL
    assert by["blk-17x512-pdt-cut-f32"]["flags"] == R.PDT
    for n in (33, 37):
        assert {c["flags"] for c in R.CASES if c["family"] == "wo" and
                c["nchan"] == n} == {R.PD, R.PDTA}
    for n in R.ALL_MASKS_ON_HOST:
        assert n in by
    # the swizzled block map: 32-channel blocks, a multiple of 8 of them
    assert len(R.SWIZZLED) == 5
    for n in R.SWIZZLED:
        assert by[n]["nchan"] % 32 == 0 and by[n]["nchan"] // 32 % 8 == 0
    assert by["swz-256x100-pd-cut-f32"]["mom_x"] is True
    # estimated and given errors both occur
    given = [R.inputs(c)["errs"] is not None for c in R.CASES
             if c["nbin"] <= 512]
    assert any(given) and not all(given)


def test_warm_stride_restates_k_tr_init():
    assert [R.warm_stride(n) for n in (64, 100, 255, 256, 257, 511, 512, 513,
                                       1024, 2048, 4096)] == \
        [1, 1, 2, 2, 2, 4, 4, 4, 8, 16, 16]


@pytest.mark.parametrize("nchan", sorted({c["nchan"] for c in R.CASES}))
def test_masks(nchan):
    for sub in {1, R.warm_stride(nchan)}:
        m = R.masks(nchan, sub)
        assert m.shape == (4, nchan) and m[0].all()
        assert (m.sum(axis=1) >= 2).all(), m.sum(axis=1)
        assert not m[1:].all(axis=1).any()
        if nchan >= 8:
            assert not m[1, 0] and not m[1, -1]
            assert abs((~m[1]).sum() - 0.2 * nchan) <= 3
        grp = np.arange(nchan) // 64
        if nchan > 64:
            # every group the warm start evaluates ((n >> 6) % sub == 0) is
            # empty; the leading 32-channel blocks are gone
            if sub > 1:
                assert not m[2][grp % sub == 0].any()
            assert not m[2][:64].any() and m[2][64:128].all()
        else:
            assert m[2][:(nchan + 1) // 2].all() and \
                not m[2][(nchan + 1) // 2:].any()
        # one live row per 8-row round, and the last
        assert m[3, -1] and m[3, ::8].all()
        assert m[3].sum() == len(range(0, nchan, 8)) + ((nchan - 1) % 8 != 0)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_template_cutoffs(name):
    """"cut": k_model_cut cuts, by different amounts in different 32-channel
    blocks, and at 2048 bins below the harmonics the fused guess holds;
    "full": no channel is cut (the guess goes through k_dsum_w)."""
    c = R.case(name)
    model, freqs = R.template(c["template"], c["nchan"], c["nbin"])
    assert model.shape == (c["nchan"], c["nbin"])
    assert np.all(np.diff(freqs) > 0)
    nharm = c["nbin"] // 2 + 1
    kc = R.kc(model)
    if c["template"] == "full":
        assert np.all(kc == nharm)
        return
    if c["nbin"] >= 1000:
        assert kc.max() < nharm
    blocks = [kc[i:i + 32].max() for i in range(0, c["nchan"], 32)]
    if c["nbin"] == 2048:
        assert kc.max() < R.GUESS_HARMONICS
        if c["nchan"] > 32:
            assert len(set(blocks)) > 1, blocks


def _well_posed(c, i):
    b = R.inputs(c)
    o = R.oracle_fit(c, i)
    assert o["return_code"] == 2, (c["name"], i, o["return_code"])
    assert len(o["scales"]) == b["keep"][i].sum()
    assert o["dof"] == b["keep"][i].sum() * (c["nbin"] - 1) - sum(c["flags"])
    o2 = R.oracle_refit(c, i, o)
    assert o2["return_code"] == 2
    dev = G.param_deviation_sigma(o2, o, b["P"], b["scat"])
    assert dev.max() < 1e-3, (c["name"], i, dev)
    return dev.max()


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_oracle_fit_is_well_posed(name):
    """The oracle converges (return code 2), and restarted from its own
    solution plus 1e-2 sigma in every fitted parameter it lands within 1e-3
    sigma of it: one minimum, sharply defined, for the device to be compared
    with at 1e-2 sigma.  All four masks for ragged.ALL_MASKS_ON_HOST, the
    unmasked sub-int for the rest (test_gpu_ragged.py asserts the return
    code of every sub-int it compares)."""
    c = R.case(name)
    for i in (range(4) if name in R.ALL_MASKS_ON_HOST else (0,)):
        _well_posed(c, i)
