"""Ragged channel counts and per-sub-int masks on every fit kernel family,
against the f64 oracle on host-built inputs (tests/ragged.py; the host
side of the same cases: tests/test_ragged_inputs.py).

Each case is ONE engine.fit_batch call on four sub-integrations that differ
in their channel masks (none; a random 20 % plus both band edges; whole
64-channel groups, those of the k_pass warm start among them; one channel
in eight), compared sub-int by sub-int with the oracle's fit of the kept
channels.  Bars: the project's (goldens.SIGMA_TOL, goldens.RCHI2_RTOL) and
the per-channel forms of test_gpu_fullshape.py."""
import numpy as np
import pytest

import goldens as G
import ragged as R

pytestmark = pytest.mark.gpu

SIG, RCHI2 = G.SIGMA_TOL, G.RCHI2_RTOL


def _compare(c, r, j, i):
    """Row j of the device output r against the oracle's fit of sub-int i."""
    b = R.inputs(c)
    return R.compare_row("RAGGED %s sub %d" % (c["name"], i), (c["name"], i),
                         r, j, R.oracle_fit(c, i), b["keep"][i], b["P"],
                         b["scat"])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_ragged_batch_matches_oracle(name):
    """A partial last channel tile and masks that empty whole tiles, in one
    batch: k_xspec_w2 + k_moments with the guess in the spectrum pass (f32
    and f64 rows; 250 channels: 8 blocks, swizzled, the last of 26) and
    through k_dsum_w, the fused k_xmom_g, forced moments from X, k_xspec_w +
    k_pass, the k_pass warm start at strides 2 and 4 with a one-channel
    last group, the mixed-radix and odd-nbin wave passes (unpaired rows),
    the block-FFT k_xspec (fewer than 32 channels; 4096 and 128 bins),
    rows past the LDS transforms, and 256 channels (8 spectrum blocks: the
    XCD-aware block map, mode 1) on k_xspec_w, k_xspec_wm, k_xspec_wo,
    k_xspec and k_xspec_any.  (Mode 2 of the block map needs more than 32 MB
    of model spectra: the full-shape scattering parity check covers it.)"""
    c = R.case(name)
    r = R.device_fit(c)
    for i in range(R.inputs(c)["nsub"]):
        _compare(c, r, i, i)


@pytest.mark.parametrize("name", ["w2_guess-250x2048-pd-cut-f32",
                                  "warm-257x256-pdta-cut-f32"] + R.SWIZZLED)
def test_ragged_single_equals_batch(name):
    """Each sub-int fitted alone is bitwise the batch's (as
    test_batch_equals_single_and_is_deterministic at 64 channels), with a
    ragged last block and differing masks; the 256-channel cases: on the
    swizzled block map, which a single sub-int takes as well."""
    c = R.case(name)
    full = R.device_fit(c)
    for i in range(R.inputs(c)["nsub"]):
        one = R.device_fit(c, [i])
        for k in ("results", "scales", "scale_errs", "channel_snrs",
                  "covariance"):
            np.testing.assert_array_equal(one[k][0], full[k][i],
                                          err_msg="%s sub %d" % (k, i))
