"""The host-side argument checks of the four Gaussian entry points, called
through ctypes with pointers that are never dereferenced: a refused call
stops before any copy or launch.  With a live context the code and the
ppf_last_error text are read; with ctx = NULL (no device) only the code."""
import ctypes

import numpy as np

from pulseportraiture_amd import _lib

_ONE = ctypes.c_void_p(8)       # a non-NULL pointer nothing reads


def live_context():
    """The device's context where the machine has a device, else None; with
    a device a failing ppf_create is an error, not a reason to pin less."""
    import torch
    return _lib.context(0) if torch.cuda.is_available() else None


def call(entry, ctx, nrow=1, nchan=2, nbin=64, ngauss=1, code=b"000", njoin=2,
         join_id=(0, 1), nfree=2, free_idx=(0, 2), delta=(1e-8, 1e-8)):
    """(return code, last error text or None) of one entry point: 'port',
    'port_join', 'lsq' or 'lsq_join'.  join_id, free_idx and delta are host
    arrays, read by the checks."""
    lib = _lib.load()
    ji = np.array(join_id, dtype=np.int32)
    fi = np.array(free_idx, dtype=np.int32)
    dl = np.array(delta, dtype=np.float64)
    head = (ctx, nrow, nchan, nbin, ngauss, code, _ONE, _ONE, _ONE, _ONE)
    join = (njoin, ji.ctypes.data, _ONE, _ONE)
    lsq = (nfree, fi.ctypes.data, dl.ctypes.data, _lib.PPF_F64, _ONE, _ONE,
           _ONE, _ONE, 1 << 30, None)
    if entry == "port":
        rc = lib.ppf_gauss_portrait_batch(*head, _ONE, None)
    elif entry == "port_join":
        rc = lib.ppf_gauss_portrait_join_batch(*head, *join, _ONE, None)
    elif entry == "lsq":
        rc = lib.ppf_gauss_lsq_batch(*head, *lsq)
    else:
        rc = lib.ppf_gauss_lsq_join_batch(*head, *join, *lsq)
    if ctx is None or rc == _lib.PPF_OK:
        return rc, None
    return rc, lib.ppf_last_error(ctx).decode()


def check(entry, want_rc, want_text, null_rc=None, **kw):
    """One refused call: code and text with a live context; the code alone
    (null_rc where the NULL context is looked at first) without one."""
    ctx = live_context()
    rc, text = call(entry, ctx, **kw)
    if ctx is None:
        assert rc == (want_rc if null_rc is None else null_rc), (entry, kw)
    else:
        assert (rc, text) == (want_rc, want_text), (entry, kw)
