"""Perceptual path length, the parts that need no GPU: ``filtered_mean`` against its definition, the torch ``slerp`` / ``lerp`` /
``normalize`` of ideas_amd.ppl in f64 against what the reference's functions computed in f64 (tests/golden/ppl.npz, stored as
float64), the batch split, the ops' refusal of CPU tensors, the header, and ``--help`` of the two command lines."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, Golden, rel_err


@pytest.fixture(scope="module")
def gold():
    return Golden("ppl.npz")


def _by_definition(values):
    """The mean of the values within [sorted[floor(0.01 (n - 1))], sorted[ceil(0.99 (n - 1))]]."""
    s = sorted(float(v) for v in values)
    n = len(s)
    lo, hi = s[math.floor(0.01 * (n - 1))], s[math.ceil(0.99 * (n - 1))]
    kept = [v for v in s if lo <= v <= hi]
    return sum(kept) / len(kept), len(kept)


@pytest.mark.parametrize("n", (1, 2, 100, 101))
def test_filtered_mean_follows_its_definition(n):
    from ideas_amd.ppl import filtered_mean
    rng = np.random.RandomState(n)
    d = rng.rand(n).astype(np.float32) * 3
    want, kept = _by_definition(d)
    assert kept == {1: 1, 2: 2, 100: 100, 101: 99}[n]         # n = 101: ranks 1 .. 99; up to 100 values the two cuts are the ends
    assert filtered_mean(d) == pytest.approx(want, rel=1e-6)
    assert filtered_mean(list(d)) == pytest.approx(want, rel=1e-6)


def test_filtered_mean_keeps_ties_at_the_cut():
    from ideas_amd.ppl import filtered_mean
    # 201 values: the cuts are ranks 2 and 198.  Three values tie at the lower cut (ranks 0 .. 2) and three at the upper one
    # (198 .. 200), so nothing is dropped; with distinct ends two values go on either side.
    d = np.array([1.0] * 3 + list(np.linspace(2.0, 3.0, 195)) + [4.0] * 3, np.float32)
    want, kept = _by_definition(d)
    assert kept == 201 and filtered_mean(d) == pytest.approx(want, rel=1e-6)
    d2 = np.array([0.0, 0.5] + list(d[2:-2]) + [5.0, 9.0], np.float32)
    want2, kept2 = _by_definition(d2)
    assert kept2 == 197 and filtered_mean(d2) == pytest.approx(want2, rel=1e-6)
    assert filtered_mean(np.random.RandomState(0).permutation(d2)) == pytest.approx(want2, rel=1e-6)


def test_torch_forms_against_the_reference_in_f64(gold):
    from ideas_amd import ppl as P
    from ideas_amd.op.ppl import path_endpoints_composition
    meta = gold.json("meta")["interp"]
    assert meta["cases"] == [[d, b] for d in (32, 100, 512) for b in (1, 3)]
    for d, b in meta["cases"]:
        tag = f"interp/{d}_{b}"
        lat, t = gold.t(f"{tag}/lat").double(), gold.t(f"{tag}/t").double()
        assert gold.z[f"{tag}/slerp"].dtype == np.float64 and tuple(lat.shape) == (2 * b, d)
        assert rel_err(P.normalize(lat), gold.t(f"{tag}/normalize")) < 1e-12
        a, bb = lat[::2], lat[1::2]
        for name, f in (("slerp", P.slerp), ("lerp", P.lerp)):
            got = torch.stack([f(a, bb, t[:, None]), f(a, bb, t[:, None] + meta["eps"])], 1).view(2 * b, d)
            e = rel_err(got, gold.t(f"{tag}/{name}"))
            assert e < 1e-12, (tag, name, e)
            assert torch.equal(path_endpoints_composition(lat, t, meta["eps"], name), got)
        unit = P.slerp(a, bb, t[:, None]).pow(2).sum(-1)
        assert float((unit - 1).abs().max()) < 1e-12


def test_slerp_of_identical_ends_is_nan():
    """No clamp, as in the reference.  Ends whose normalisation is exact (four equal entries: norm 3, direction 0.5) have the dot
    product 1 exactly, so c = 0 / 0.  (A dot product that ROUNDS below 1 gives a finite row without meaning instead.)"""
    from ideas_amd.ppl import slerp
    a = torch.zeros(2, 8, dtype=torch.float64)
    a[0, :4], a[1, 2:6] = 1.5, -1.5
    assert bool(torch.isnan(slerp(a, a.clone(), torch.full((2, 1), 0.25, dtype=torch.float64))).all())


def test_batch_split():
    from ideas_amd.ppl import batch_sizes
    assert batch_sizes(10, 4) == [4, 4, 2]
    assert batch_sizes(8, 4) == [4, 4, 0]                     # the reference's zero-sized last batch (compute_ppl skips it)
    assert batch_sizes(3, 4) == [3]
    assert batch_sizes(5000, 64) == [64] * 78 + [8]


def test_compute_ppl_draws_in_the_references_order_and_skips_the_empty_batch(monkeypatch):
    """``compute_ppl`` on stand-ins for the generator and ``path_distances``: per batch ``make_noise``, ``randn([2 b, D])``,
    ``rand(b)``; no call for the zero-sized batch; the result is ``filtered_mean`` of all the distances."""
    from ideas_amd import ppl as P
    calls = []

    class G:
        style_dim = 5
        input = type("I", (), {"input": torch.zeros(1)})()

        def make_noise(self):
            calls.append("make_noise")
            return ["noise"]
    o_randn, o_rand = torch.randn, torch.rand

    def randn(*a, **k):
        calls.append(("randn", list(a[0])))
        return o_randn(*a, **k)

    def rand(*a, **k):
        calls.append(("rand", a[0]))
        return o_rand(*a, **k)

    def path_distances(g, percept, inputs, lerp_t, noise, **kw):
        assert noise == ["noise"] and tuple(inputs.shape) == (2 * lerp_t.shape[0], 5) and kw["space"] == "w" and kw["eps"] == 1e-2
        return lerp_t.clone()
    monkeypatch.setattr(torch, "randn", randn)
    monkeypatch.setattr(torch, "rand", rand)
    monkeypatch.setattr(P, "path_distances", path_distances)
    got = P.compute_ppl(G(), None, 8, 4, "w", 1e-2, False, seed=3)
    assert calls == ["make_noise", ("randn", [8, 5]), ("rand", 4)] * 2
    torch.manual_seed(3)
    want = []
    for _ in range(2):
        o_randn([8, 5])
        want.append(o_rand(4).numpy())
    assert got == pytest.approx(P.filtered_mean(np.concatenate(want)), rel=1e-7)
    calls.clear()
    P.compute_ppl(G(), None, 6, 4, "w", 1e-2, False, seed=3)
    assert calls == ["make_noise", ("randn", [8, 5]), ("rand", 4), "make_noise", ("randn", [4, 5]), ("rand", 2)]


def test_ops_refuse_cpu_tensors():
    import ideas_amd.op as op
    assert op.path_endpoints is not None and op.pair_prepare is not None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.path_endpoints(torch.randn(4, 8), torch.rand(2), 1e-4, "lerp")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.path_endpoints(torch.randn(4, 8, dtype=torch.float64), torch.rand(2, dtype=torch.float64), 1e-4, "slerp")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.pair_prepare(torch.randn(2, 3, 8, 8), (0, 0, 8, 8), (8, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match="mode"):
        op.path_endpoints(torch.randn(4, 8), torch.rand(2), 1e-4, "nlerp")
    with pytest.raises(RuntimeError, match=r"\[2B, D\]"):
        op.path_endpoints(torch.randn(3, 8), torch.rand(2), 1e-4, "lerp")


def test_header_declares_both_functions_and_the_binding_types_them():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    for name in ("ideas_path_endpoints", "ideas_pair_prepare"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define IDEAS_PATH_MAX_DIM (\d+)", hdr).group(1)) == _lib.PATH_MAX_DIM
    assert (int(re.search(r"#define IDEAS_PATH_LERP (\d+)", hdr).group(1)), int(re.search(r"#define IDEAS_PATH_SLERP (\d+)", hdr).group(1))) \
        == (_lib.PATH_LERP, _lib.PATH_SLERP)


@pytest.mark.parametrize("script", ("ppl.py", "generate.py"))
def test_command_lines_print_their_help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--seed" in r.stdout and ("--space" if script == "ppl.py" else "--truncation_mean") in r.stdout
