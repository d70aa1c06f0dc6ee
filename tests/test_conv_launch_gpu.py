"""GPU: the split-K plans of the weight-gradient launchers at the device's real occupancy (csrc/conv_launch.hpp)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_splitk_plans as G  # noqa: E402
from test_host_logic import splitk_plan_rows  # noqa: E402

pytestmark = pytest.mark.gpu


def test_splitk_plans_fill_whole_waves_at_the_measured_occupancy(monkeypatch):
    """With the slot count the library's own device query reports (resident blocks per CU x CUs), the f32, split-bf16 and Winograd
    weight gradients launch a whole number of waves of blocks whenever the grid exceeds one wave and a split count giving whole
    waves exists -- the property the re-balance of conv_launch.hpp is there for -- and the plans are still those of the
    transcription in tests/golden/make_golden_splitk_plans.py at that slot count."""
    from ideas_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    cases = sorted({tuple(c[:6]) + (0,) for c in np.load(os.path.join(ROOT, "tests", "golden", "splitk_plans.npz"))["cases"].tolist()})
    seen = []
    real = G._waves_rebalance
    monkeypatch.setattr(G, "_waves_rebalance", lambda *a: (seen.append(a), real(*a))[1])
    whole = 0
    for name in ("igemm", "wino", "b3_wgrad"):
        site, scaled, plan, admits = G.SITES[name]
        sel = [c for c in cases if admits(*c)]
        rows = splitk_plan_rows(lib, sel, site, scaled)
        assert (rows[:, 3] > 0).all(), name
        print(name, "slots on this device:", sorted(set(rows[:, 3].tolist())))
        for c, row in zip(sel, rows.tolist()):
            slots = row[3]
            del seen[:]
            assert tuple(plan(*c[:6], slots)) == tuple(row), (name, c)
            (P, per0, splits0, tiles, _, step), = seen
            blocks = tiles * row[0]
            waves = tiles * splits0 // slots
            if waves >= 1 and (waves * slots) % tiles == 0:
                s = waves * slots // tiles
                if G.cdiv(P, G.cdiv(G.cdiv(P, s), step) * step) == s:       # `s` shares of whole steps exist
                    assert blocks == waves * slots, (name, c, row)
                    whole += 1
    assert whole > 100
