#!/usr/bin/env python3
"""Writes tests/golden/jpeg_pinned.npz: shape, SHA-256 and first 16 values of out, y and coef of every case of
tests/test_jpeg_pinned_gpu.py, from the library that is loaded (IDEAS_HIP_LIB, else ideas_amd/libideas_hip.so).

Run on a GPU with the library of the commit whose results are to be pinned (built into a directory of its own):
    IDEAS_HIP_LIB=<parent build>/libideas_hip.so python tests/golden/make_golden_jpeg_pinned.py [out.npz]
Every case runs twice and must give the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_jpeg_pinned_gpu as T  # noqa: E402


def main():
    from ideas_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    print("library:", _lib.LIB_PATH)
    d = {}
    for name in sorted(T.CASES):
        a, b = T.run_case(name), T.run_case(name)
        assert [x[1] for x in a] == [x[1] for x in b], name + ": two runs differ"
        d[name + "/n"] = np.int64(len(a))
        for i, (shape, sha, head) in enumerate(a):
            k = "%s/%d" % (name, i)
            d[k + "/shape"] = np.array(shape, dtype=np.int64)
            d[k + "/sha256"] = np.frombuffer(bytes.fromhex(sha), dtype=np.uint8)
            d[k + "/head"] = head.astype(np.float32)
    np.savez_compressed(out, **d)
    print("wrote", out, len(T.CASES), "cases", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
