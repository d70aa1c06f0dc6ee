#!/usr/bin/env python3
"""Writes tests/golden/fir_pinned.npz: shape, SHA-256 and first 16 values of every pinned output of the cases of
tests/test_fir_pinned_gpu.py, from the library that is loaded (IDEAS_HIP_LIB, else ideas_amd/libideas_hip.so).

Run on a GPU with the library of the commit whose results are to be pinned:
    IDEAS_HIP_LIB=<that library> python tests/golden/make_golden_fir_pinned.py [out.npz]
Every case runs twice and must give the same bytes, and every output is first checked against the f64 oracle
(oracle.torch_ref.upfirdn2d, followed in f64 by the fused stage or the residual where the case has one) at the suite's
tolerances: 2e-6 for f32, 6e-3 for bf16 and f16.  The bias gradient of the fused cases is not pinned (f32 atomics in varying
order); it is checked against the f64 sum of the pinned y, as the test does."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_fir_pinned_gpu as T  # noqa: E402
from conftest import rel_err  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    keys, shapes, shas, heads = [], [], [], []
    for name in sorted(T.CASES):
        (a, outs, refs), (b, _, _) = T.run_case(name), T.run_case(name)
        a, b = T.pinned(name, a), T.pinned(name, b)
        assert [x[1] for x in a] == [x[1] for x in b], name + ": two runs differ"
        tol = T.TOL[[k for k in T.TOL if "_" + k in name][0]]
        errs = [rel_err(o, r) for o, r in zip(outs, refs)]
        print(name, [x[0] for x in a], a[0][1][:16], "oracle", " ".join("%.3g" % e for e in errs), flush=True)
        assert all(e < tol for e in errs[:len(a)]), (name, errs, tol)
        if name in T.FUSED:
            assert errs[2] < T.bias_grad_tol(name), (name, errs[2])
        for i, (shape, sha, head) in enumerate(a):
            assert len(shape) == 4 and len(head) == 16
            keys.append("%s/%d" % (name, i))
            shapes.append(shape)
            shas.append(np.frombuffer(bytes.fromhex(sha), dtype=np.uint8))
            heads.append(head)
    np.savez_compressed(out, keys=np.array(keys), shape=np.array(shapes, dtype=np.int64), sha256=np.stack(shas),
                        head=np.stack(heads).astype(np.float64))
    print("wrote", out, os.path.getsize(out), "bytes,", len(T.CASES), "cases")

if __name__ == "__main__":
    main()
