"""Section cycle profile of k_postfit from a PPF_PF_PROF build (thread 0 of
every workgroup, shader-clock cycles summed over workgroups):
    tools/build_variant.sh pfprof -DPPF_PF_PROF=1
    PPFIT_LIB=varlib/libppfit_pfprof.so python tools/pfprof.py [bench args]
(default bench args: the headline shape, two steps)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch  # noqa: F401  (the HIP runtime comes up through torch first)
    from pulseportraiture_amd import _lib
    _lib.load()
    dll = ctypes.CDLL(os.environ["PPFIT_LIB"])
    get = dll.ppf_debug_pfprof
    get.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = np.zeros(8, dtype=np.uint64)
    args = sys.argv[1:] or ["--steps", "2", "--warmup", "1", "--cpu-sample", "0"]
    sys.argv = ["bench.py"] + args
    import bench
    get(out.ctypes.data, 1)
    bench.main()
    get(out.ctypes.data, 1)
    names = ["Sd sum, gates", "zero-cov loop", "nz_solve (t0)", "covariance loop",
             "inversion (t0)", "scales loop", "record (t0)"]
    tot = float(out[:7].sum())
    for i, nm in enumerate(names):
        print("%-16s %14d  %5.1f%%" % (nm, out[i], 100.0 * out[i] / tot))


if __name__ == "__main__":
    main()
