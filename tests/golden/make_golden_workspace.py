#!/usr/bin/env python
"""Golden tables of the workspace queries, checked byte for byte by
tests/test_abi.py.  The queries need no device.

fit_workspace.json: ppf_fit_workspace_bytes over a grid of descriptors.
long_workspace.json: the three long-transform queries over LONG_NROWS x
LONG_NBIN (zeros for the shapes they refuse included).

The tables pin the workspace layouts against refactors of fit_layout and of
the long transforms' plans, so they are generated from a build of the commit
BEFORE the change under test, never from the tree being tested:

    PPFIT_LIB=/path/to/parent/pulseportraiture_amd/lib/libppfit.so \\
        python tests/golden/make_golden_workspace.py

Each fit entry is [nbin, nchan, nsub, nmodel, guess, guess_Ns, options,
x_subints, bytes]; each long entry is [nrows, nbin, noise_long,
noise_fit_long, rotate_long(ref_len 0), rotate_long(ref_len 1)].
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pulseportraiture_amd import _lib  # noqa: E402

NBIN = (64, 1000, 1001, 1024, 2048, 4096, 8194, 16384)
NCHAN = (1, 33, 512)
NSUB = (1, 10)
NMODEL = (1, 3)
GUESS = ("off", 100, "nbin")          # off, guess_Ns = 100, guess_Ns = nbin
OPTIONS = (0, _lib.OPT_NO_X, _lib.OPT_MOM_X, _lib.OPT_FUSED_MOM)
X_SUBINTS = (0, 2)
# 600 and 70000 rows put several nbin past one 256 MB chunk
LONG_NROWS = (0, 1, 3, 600, 70000)
LONG_NBIN = (1, 2, 3, 33, 4097, 8186, 8194, 16384, 1 << 20, 511 * 1023,
             1 << 25, (1 << 25) + 2)


def grid():
    for nbin, nchan, nsub, nmodel, g, opt, xs in itertools.product(
            NBIN, NCHAN, NSUB, NMODEL, GUESS, OPTIONS, X_SUBINTS):
        guess = 0 if g == "off" else 1
        guess_Ns = 0 if g == "off" else (nbin if g == "nbin" else g)
        yield nbin, nchan, nsub, nmodel, guess, guess_Ns, opt, xs


def workspace_bytes(lib, nbin, nchan, nsub, nmodel, guess, guess_Ns, options,
                    x_subints):
    d = _lib.FitDesc()
    d.nbin, d.nchan, d.nsub, d.nmodel = nbin, nchan, nsub, nmodel
    d.guess, d.guess_Ns = guess, guess_Ns
    d.options, d.x_subints = options, x_subints
    return int(lib.ppf_fit_workspace_bytes(ctypes.byref(d)))


def long_bytes(lib, nrows, nbin):
    return [int(lib.ppf_noise_long_workspace_bytes(nrows, nbin)),
            int(lib.ppf_noise_fit_long_workspace_bytes(nrows, nbin)),
            int(lib.ppf_rotate_long_workspace_bytes(nrows, nbin, 0)),
            int(lib.ppf_rotate_long_workspace_bytes(nrows, nbin, 1))]


def write(name, entries):
    out = os.path.join(HERE, name)
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":"))
                                   for e in entries) + "\n]\n")
    print("%d entries from %s -> %s" % (len(entries), _lib.LIB_PATH, out))


def main():
    lib = _lib.load()
    write("fit_workspace.json",
          [list(g) + [workspace_bytes(lib, *g)] for g in grid()])
    write("long_workspace.json",
          [[nrows, nbin] + long_bytes(lib, nrows, nbin)
           for nrows, nbin in itertools.product(LONG_NROWS, LONG_NBIN)])


if __name__ == "__main__":
    main()
