#!/usr/bin/env python3
"""Writes tests/golden/png_pinned.npz: the files tests/png_ref.py makes of its fixtures (seeded, made here from nothing), so that
tests/test_png_file.py notices a silent change of the contract of "The PNG file, written" (include/ideas_hip.h).

    python tests/golden/make_golden_png.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_ref as R  # noqa: E402


def main():
    out = {}
    for name in R.FIXTURES:
        data, _ = R.png_file(R.fixture(name))
        out["file/" + name] = np.frombuffer(data, np.uint8)
        print(name, R.FIXTURES[name], len(data), "bytes")
    path = os.path.join(HERE, "png_pinned.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
