"""FID on the GPU: ``op.pool3x3`` / ``op.global_avg_pool`` (csrc/pool.hip), ``FeatureStats`` (csrc/feature_stats.hip), the
rectangular-padding convs, ``ideas_amd.inception.InceptionV3`` and ``ideas_amd.fid`` against the reference's own code
(tests/golden/fid.npz, written by tests/golden/make_golden_fid.py on the seeded torchvision stand-in of tests/fid_ref.py), and the two
command lines.

Tolerances.  Ops: the max pools are exact; the average, the global average and the convs 1e-5 of the largest element (DESIGN.md
"Tolerances"), bf16 tensors ``close_bf16``.  Networks: the rule of tests/test_non_leaking_gpu.py, ``max(1e-5, 4 x the reference's own
f32-from-f64 deviation)``.  The deviations tests/golden/make_golden_fid.py printed (and stored as ``*/f32_dev`` = [features, block
sums, block slices]): ``up`` 2.0e-7, 1.5e-7, 8.5e-7; ``same`` 1.6e-7, 6.9e-8, 6.9e-7; ``down`` 2.4e-6, 1.4e-6, 4.5e-6; ``norm01`` 2.8e-7,
1.8e-7, 5.5e-7; generator features 3.3e-7 (truncation 1) and 2.7e-7 (0.7); the 4-dimensional end-to-end distance 1.1e-6; statistics:
mean 2.0e-7 (numpy adds f32 features in f32), covariance 5.9e-16 (numpy's own f64 evaluation against long double).

``FeatureStats`` against numpy in f64, elementwise, from the summation model with no fitted constant (u = 2^-53, A = |X|^T |X|,
a = sum_n |x_n|): each of the kernel's and numpy's N-term sums is within N u of its absolute sum, so

    |gram - X^T X| <= 4 N u A                    |sum - sum_n x_n| <= 4 N u a
    |cov - np.cov| <= u ((5 n + 7) A + (11 n + 15) a a^T / n) / (n - 1)

the last one propagating the two bounds through ``(gram - sum sum^T / n) / (n - 1)`` (4 n u A; 2 x 4 n u a a^T / n; 3 u (A + a a^T /
n) for the three host operations) plus numpy's own centred evaluation ((n + 4) u |Xc|^T |Xc| with |Xc|^T |Xc| <= A + 3 a a^T / n).
"""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, Golden, rel_err
from test_bf16_gpu import close_bf16
import fid_ref as FR

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
TOL = 1e-5
U = 2.0 ** -53
DTYPES = (torch.float32, BF)
_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")


@pytest.fixture(scope="module")
def gold():
    return Golden("fid.npz")


@pytest.fixture(scope="module")
def P():
    from ideas_amd.op import pool
    return pool


def fmt(t, layout):
    return t.contiguous(memory_format=CL) if layout == "nhwc" else t.contiguous()


def _ref_pool(x64, mode, P):
    return P.pool3x3_composition(x64, mode)


# ------------------------------------------------------------------------------------------------- op.pool3x3
# 16-byte vectors (8, 64, 288 channels; bf16: 8 | C), the scalar channel path (5, 3), one window (3x3), W < one run, several runs
# per row and several blocks (35 x 35 x 288)
POOL_CASES = [(2, 8, 7, 7), (1, 5, 3, 3), (2, 64, 9, 4), (1, 3, 4, 5), (1, 288, 35, 35)]


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids)
def test_pool3x3(P, case, dtype, layout):
    """The three modes against the F.* calls on the CPU in f64 on the same rounded operands."""
    g = torch.Generator().manual_seed(3 + sum(case))
    x = torch.randn(*case, generator=g).to(dtype)
    xd = fmt(x.cuda(), layout)
    for mode in P.MODES:
        ref = _ref_pool(x.double(), mode, P)
        y = P.pool3x3(xd, mode)
        assert y.dtype == dtype and tuple(y.shape) == tuple(ref.shape) and y.is_contiguous(memory_format=CL)
        if mode != P.AVG_S1P1_VALID:
            assert torch.equal(y.double().cpu(), ref), mode
        elif dtype == BF:
            close_bf16(y, ref, "avg")
        else:
            err = rel_err(y, ref)
            print(case, layout, "avg rel err", err)
            assert err <= TOL


def test_pool3x3_avg_divisors_are_the_in_image_taps(P):
    """An all-ones image stays all ones (4 / 6 / 9 taps over 4 / 6 / 9), where the zero-padded average would give 4/9 at a corner."""
    for shape in ((1, 8, 5, 6), (1, 3, 1, 1), (2, 5, 2, 9), (1, 8, 1, 4)):
        y = P.pool3x3(torch.ones(*shape, device="cuda"), P.AVG_S1P1_VALID)
        assert torch.equal(y.cpu(), torch.ones(*shape)), shape


def test_pool3x3_max_s1p1_padding_never_wins(P):
    """An all-negative input: a zero (or any finite) padding value would be the maximum along the border."""
    g = torch.Generator().manual_seed(21)
    for dtype in DTYPES:
        x = (-1.0 - torch.rand(2, 8, 6, 5, generator=g)).to(dtype)
        y = P.pool3x3(x.cuda(), P.MAX_S1P1)
        assert float(y.max()) < 0 and torch.equal(y.double().cpu(), F.max_pool2d(x.double(), 3, 1, 1))
        z = torch.full((1, 5, 4, 4), -float("inf"), dtype=dtype)
        assert torch.equal(P.pool3x3(z.cuda(), P.MAX_S1P1).cpu(), z)


def test_pool3x3_nan_is_the_maximum(P):
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, 8, 9, 9, generator=g)
    x[0, 2, 4, 4] = float("nan")
    x[0, 5, 0, 8] = float("nan")
    x[0, 7, 8, 0] = float("inf")
    for mode in (P.MAX_S2, P.MAX_S1P1):
        ref = _ref_pool(x, mode, P)
        for xx in (x, x[:, :5]):                                   # vector and element paths
            r = _ref_pool(xx, mode, P)
            y = P.pool3x3(xx.cuda(), mode).cpu()
            assert torch.equal(torch.isnan(y), torch.isnan(r)) and int(torch.isnan(r).sum()) >= 2
            assert torch.equal(torch.nan_to_num(y, nan=0.0), torch.nan_to_num(r, nan=0.0))
        assert int(torch.isnan(ref[0, 2]).sum()) == (4 if mode == P.MAX_S2 else 9)


def test_pool3x3_is_bitwise_reproducible_and_layout_independent(P):
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 24, 19, 13, generator=g).cuda()
    for dtype in DTYPES:
        for mode in P.MODES:
            a = P.pool3x3(x.to(dtype), mode)
            b = P.pool3x3(x.to(dtype), mode)
            c = P.pool3x3(x.to(dtype).contiguous(memory_format=CL), mode)
            assert torch.equal(a, b) and torch.equal(a, c)
    # the element path (a view that is not 16-byte aligned) computes the vector path's values
    buf = torch.zeros(2 * 19 * 13 * 24 + 1, device="cuda")
    v = buf[1:].view(2, 19, 13, 24).permute(0, 3, 1, 2)
    v.copy_(x)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous(memory_format=CL)
    assert torch.equal(P.pool3x3(v, P.AVG_S1P1_VALID), P.pool3x3(x, P.AVG_S1P1_VALID))


def test_pool3x3_rejects_and_compositions(P):
    x = torch.randn(1, 4, 2, 7, device="cuda")
    with pytest.raises(RuntimeError, match="smaller than the 3x3 window"):
        P.pool3x3(x, P.MAX_S2)
    with pytest.raises(RuntimeError, match="smaller than the 3x3 window"):
        P.pool3x3(x.permute(0, 1, 3, 2), P.MAX_S2)
    assert tuple(P.pool3x3(x, P.MAX_S1P1).shape) == (1, 4, 2, 7)
    with pytest.raises(RuntimeError, match="mode"):
        P.pool3x3(x, 3)
    with pytest.raises(RuntimeError, match="4-D"):
        P.pool3x3(x[0], P.MAX_S1P1)
    xg = torch.randn(1, 4, 5, 5, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        P.pool3x3(xg, P.MAX_S1P1)
    with pytest.raises(RuntimeError, match="forward-only"):
        P.global_avg_pool(xg)
    with torch.no_grad():
        assert not P.pool3x3(xg, P.MAX_S1P1).requires_grad
    with pytest.raises(RuntimeError, match="float32 and bfloat16"):
        P.pool3x3(torch.zeros(1, 4, 5, 5, device="cuda", dtype=torch.int32), P.MAX_S1P1)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(2, 8, 6, 7, generator=g)
    for dtype in (torch.float16, torch.float64):                 # the torch compositions
        for mode in P.MODES:
            y = P.pool3x3(x.to(dtype).cuda(), mode)
            assert y.dtype == dtype and rel_err(y, _ref_pool(x.to(dtype).double(), mode, P)) <= (1e-3 if dtype == torch.float16 else 1e-12)
        y = P.global_avg_pool(x.to(dtype).cuda())
        assert y.dtype == dtype and tuple(y.shape) == (2, 8, 1, 1)


# ------------------------------------------------------------------------------------------------- op.global_avg_pool
@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", [(2, 2048, 8, 8), (3, 5, 3, 7), (1, 8, 1, 1)], ids=_ids)
def test_global_avg_pool(P, case, dtype, layout):
    g = torch.Generator().manual_seed(31 + sum(case))
    x = torch.randn(*case, generator=g).to(dtype)
    ref = F.adaptive_avg_pool2d(x.double(), 1)
    xd = fmt(x.cuda(), layout)
    y = P.global_avg_pool(xd)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(ref.shape)
    err = rel_err(y, ref)
    print(case, dtype, layout, "rel err", err)
    assert err <= TOL
    assert torch.equal(y, P.global_avg_pool(xd))


# ------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_checks_run_before_any_launch():
    """NULL pointers, non-positive sizes, unknown modes and dtypes without a kernel are answered by the checks in front of the launch
    (the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)

    def pool(y=a, x=a, B=2, C=8, H=4, W=4, mode=_lib.POOL_MAX_S2, dtype=_lib.F32):
        return lib.ideas_pool3x3_fwd(y, x, B, C, H, W, mode, dtype, None)

    def gavg(out=a, x=a, B=2, C=8, H=4, W=4, dtype=_lib.F32):
        return lib.ideas_global_avg_pool(out, x, B, C, H, W, dtype, None)

    def stats(s=a, g=a, x=a, N=4, D=8):
        return lib.ideas_feature_stats_accum(s, g, x, N, D, None)
    for f in (pool, gavg):
        assert f(B=0) == E_SHAPE and f(C=0) == E_SHAPE and f(H=-1) == E_SHAPE and f(W=0) == E_SHAPE
        assert f(dtype=_lib.F16) == E_UNSUPPORTED and f(dtype=_lib.F64) == E_UNSUPPORTED and f(dtype=17) == E_UNSUPPORTED
        assert f(x=None) == E_NULL
    assert pool(H=2) == E_SHAPE and pool(W=2) == E_SHAPE                          # no window fits
    assert pool(H=2, y=None, mode=_lib.POOL_MAX_S1P1) == E_NULL and pool(H=1, W=1, x=None, mode=_lib.POOL_AVG_S1P1_VALID) == E_NULL
    assert pool(mode=3) == E_UNSUPPORTED and pool(mode=-1) == E_UNSUPPORTED
    assert pool(y=None) == E_NULL and gavg(out=None) == E_NULL
    assert stats(N=0) == E_SHAPE and stats(D=0) == E_SHAPE and stats(N=-3) == E_SHAPE
    assert stats(D=4097) == E_UNSUPPORTED and stats(D=4096, x=None) == E_NULL
    assert stats(s=None) == E_NULL and stats(g=None) == E_NULL and stats(x=None) == E_NULL


# ------------------------------------------------------------------------------------------------- FeatureStats
def _features(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(0.3 + torch.randn(n, d, generator=g)) * (1 + torch.rand(d, generator=g))


def _moment_bounds(x64, n_terms):
    A = np.abs(x64).T @ np.abs(x64)
    a = np.abs(x64).sum(0)
    return 4 * n_terms * U * A + 1e-300, 4 * n_terms * U * a + 1e-300, A, a


def _check_stats(st, x, what):
    x64 = x.double().numpy()
    n = x64.shape[0]
    eg, es, A, a = _moment_bounds(x64, n)
    gram, s = st.gram.cpu().numpy(), st.sum.cpu().numpy()
    dg, ds = np.abs(gram - x64.T @ x64), np.abs(s - x64.sum(0))
    print(what, "gram err / bound", float((dg / eg).max()), "sum err / bound", float((ds / es).max()))
    assert st.n == n and (dg <= eg).all() and (ds <= es).all(), what
    assert np.array_equal(gram, gram.T), what                                    # symmetric by construction
    assert (np.abs(st.mean() - x64.mean(0)) <= es / n + 2 * U * a / n + 1e-300).all(), what
    if n >= 2:
        ec = U * ((5 * n + 7) * A + (11 * n + 15) * np.outer(a, a) / n) / (n - 1) + 1e-300
        dc = np.abs(st.cov() - np.cov(x64, rowvar=False).reshape(ec.shape))
        print(what, "cov err / bound", float((dc / ec).max()))
        assert (dc <= ec).all(), what


@pytest.mark.parametrize("n", (1, 5, 33))
@pytest.mark.parametrize("d", (1, 70, 2048))
def test_feature_stats_against_numpy(d, n):
    from ideas_amd.fid import FeatureStats
    x = _features(n, d, 40 + n + d)
    st = FeatureStats(d).update(x.cuda())
    _check_stats(st, x, f"D={d} N={n}")
    again = FeatureStats(d).update(x.cuda())
    assert torch.equal(st.gram, again.gram) and torch.equal(st.sum, again.sum)   # two runs are bitwise equal
    # two updates = one update of the concatenation (the kernel continues each element's sum in index order: bitwise), so is merge
    # within the bound
    y = _features(7, d, 90 + n + d)
    both = torch.cat([x, y], 0)
    two = FeatureStats(d).update(x.cuda()).update(y.cuda())
    one = FeatureStats(d).update(both.cuda())
    _check_stats(two, both, f"D={d} N={n}+7 two updates")
    assert two.n == one.n == n + 7 and torch.equal(two.gram, one.gram) and torch.equal(two.sum, one.sum)
    merged = FeatureStats(d).update(x.cuda()).merge(FeatureStats(d).update(y.cuda()))
    _check_stats(merged, both, f"D={d} N={n}+7 merged")
    assert np.array_equal(merged.gram.cpu().numpy(), merged.gram.cpu().numpy().T)


def test_feature_stats_accepts_the_networks_shape_and_rejects_others():
    from ideas_amd.fid import FeatureStats
    x = _features(3, 16, 5)
    a = FeatureStats(16).update(x.cuda().view(3, 16, 1, 1))
    assert a.n == 3 and torch.equal(a.gram, FeatureStats(16).update(x.cuda()).gram)
    assert FeatureStats(16).update(x[:0].cuda()).n == 0
    with pytest.raises(RuntimeError, match="expected"):
        FeatureStats(8).update(x.cuda())
    with pytest.raises(RuntimeError, match="no features"):
        FeatureStats(8).mean()
    with pytest.raises(RuntimeError, match="two samples"):
        FeatureStats(16).update(x[:1].cuda()).cov()
    with pytest.raises(RuntimeError, match="merge"):
        a.merge(FeatureStats(8))
    assert FeatureStats(16).merge(a).n == 3


def test_feature_stats_match_the_references_statistics(gold):
    """np.mean / np.cov of fid.py:97-98 on the seeded [37, 2048] matrix: within 4 x the reference's own deviation from the
    extended-precision values, max-abs over max-abs (mean 2.0e-7, covariance 5.9e-16)."""
    from ideas_amd.fid import FeatureStats
    f = FR.stats_features()
    sums = gold.z["stats/f_sums"]
    assert float(f.double().sum()) == pytest.approx(sums[0], rel=1e-12) and float(f.double().abs().sum()) == pytest.approx(sums[1], rel=1e-12)
    dev_mean, dev_cov = gold.z["stats/dev"].tolist()
    st = FeatureStats(2048)
    for k in range(0, 37, 16):                                                    # batches of 16, 16 and 5
        st.update(f[k:k + 16].cuda())
    mean, cov = st.mean(), st.cov()
    assert mean.dtype == np.float64 and cov.dtype == np.float64 and cov.shape == (2048, 2048) and np.array_equal(cov, cov.T)
    mt, dt, bt = gold.z["stats/mean_true"], gold.z["stats/cov_true_diag"], gold.z["stats/cov_true_block"]
    den = float(np.abs(dt).max())
    assert den >= float(np.abs(bt).max())
    e_mean = float(np.abs(mean - mt).max() / np.abs(mt).max())
    e_cov = max(float(np.abs(np.diagonal(cov) - dt).max()), float(np.abs(cov[:64, :64] - bt).max())) / den
    print("mean err", e_mean, "bound", 4 * dev_mean, "cov err", e_cov, "bound", 4 * dev_cov)
    assert e_mean <= 4 * dev_mean and e_cov <= 4 * dev_cov
    want = gold.z["stats/cov_true_sums"]
    assert float(cov.sum()) == pytest.approx(want[0], rel=1e-9) and float(np.abs(cov).sum()) == pytest.approx(want[1], rel=1e-9)
    # and the values the reference itself computed, by its own deviation
    assert float(np.abs(mean - gold.z["stats/mean"]).max() / np.abs(mt).max()) <= 5 * dev_mean
    assert float(np.abs(np.diagonal(cov) - gold.z["stats/cov_diag"]).max()) / den <= 5 * dev_cov


# ------------------------------------------------------------------------------------------------- rectangular-padding convs
CONV_CASES = [  # kernel, padding, stride, cin, cout, (h, w)
    ((1, 7), (0, 3), 1, 32, 32, (9, 11)), ((7, 1), (3, 0), 1, 32, 32, (9, 11)),
    ((1, 3), (0, 1), 1, 48, 80, (8, 8)), ((3, 1), (1, 0), 1, 48, 80, (8, 8)),
    ((5, 5), 2, 1, 48, 64, (7, 7)),
    ((3, 3), 0, 2, 3, 32, (15, 15)), ((3, 3), 0, 2, 32, 48, (35, 35)),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k%dx%d_p%s_s%d_%d-%d" % (c[0] + (str(c[1]).replace(" ", ""),) + c[2:5]))
def test_conv2d_bias_act_rectangular_padding(case):
    import ideas_amd.op as op
    kernel, padding, stride, cin, cout, (h, w) = case
    g = torch.Generator().manual_seed(50 + cin + cout + h)
    x = torch.randn(2, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, *kernel, generator=g) * (2.0 / (cin * kernel[0] * kernel[1])) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=padding))
    with torch.no_grad():
        y = op.conv2d_bias_act(x.cuda(), wt.cuda().contiguous(memory_format=CL), b.cuda(), stride=stride, padding=padding,
                               negative_slope=0.0, scale=1.0)
        y2 = op.conv2d(x.cuda(), wt.cuda(), b.cuda(), stride=stride, padding=padding)
    assert tuple(y.shape) == tuple(ref.shape)
    err = rel_err(y, ref)
    err2 = rel_err(y2, F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=padding))
    print(case, "rel err", err, err2)
    assert err <= TOL and err2 <= TOL
    if isinstance(padding, tuple):
        with pytest.raises(RuntimeError, match="forward-only"):
            op.conv2d_bias_act(x.cuda().requires_grad_(True), wt.cuda(), b.cuda(), stride=stride, padding=padding)
        with pytest.raises(RuntimeError, match="forward-only"):
            op.conv2d(x.cuda(), wt.cuda().requires_grad_(True), padding=padding)


# ------------------------------------------------------------------------------------------------- InceptionV3
@pytest.fixture(scope="module")
def backbone(gold):
    sd = FR.backbone_state()
    meta = gold.json("meta")["backbone"]
    assert meta["seed"] == FR.BACKBONE_SEED and [[k, list(v.shape)] for k, v in sd.items()] == meta["keys"]
    sums = FR.checksums(sd)
    for k, (s, a) in meta["checksums"].items():
        assert sums[k][0] == pytest.approx(s, rel=1e-5, abs=1e-5) and sums[k][1] == pytest.approx(a, rel=1e-5), k
    return sd


@pytest.fixture(scope="module")
def net(backbone):
    from ideas_amd.inception import InceptionV3
    return InceptionV3([0, 1, 2, 3], normalize_input=False, weights=backbone).cuda()


@pytest.fixture(scope="module")
def net3(backbone):
    from ideas_amd.inception import InceptionV3
    return InceptionV3([3], normalize_input=False, weights=backbone).cuda()


def _case(gold, tag):
    x = FR.case_input(tag)
    want = gold.z[f"net/{tag}/x_sums"]
    got = np.array([[float(x[n].double().sum()), float(x[n].double().abs().sum())] for n in range(2)])
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9), "the seeded input was not remade"
    return x


@pytest.mark.parametrize("tag", list(FR.CASES), ids=str)
def test_inception_matches_the_reference(gold, net, net3, tag):
    x = _case(gold, tag)
    net.normalize_input = net3.normalize_input = FR.CASES[tag][2]
    try:
        outs = net(x.cuda())
        only = net3(x.cuda())
    finally:
        net.normalize_input = net3.normalize_input = False
    assert [tuple(o.shape) for o in outs] == [(2, 64, 73, 73), (2, 192, 35, 35), (2, 768, 17, 17), (2, 2048, 1, 1)]
    assert all(o.dtype == torch.float32 for o in outs)
    d_feat, d_sums, d_slices = gold.z[f"net/{tag}/f32_dev"].tolist()
    e_feat = rel_err(outs[3].reshape(2, -1), gold.t(f"net/{tag}/feat"))
    sums = torch.tensor([[[float(o[n].double().sum()), float(o[n].double().abs().sum())] for n in range(2)] for o in outs[:3]],
                        dtype=torch.float64)
    e_sums = rel_err(sums, gold.t(f"net/{tag}/sums"))
    e_slices = max(rel_err(FR.block_slice(outs[k]), gold.t(f"net/{tag}/slice{k}")) for k in range(3))
    print(tag, "feat", e_feat, max(TOL, 4 * d_feat), "sums", e_sums, max(TOL, 4 * d_sums), "slices", e_slices, max(TOL, 4 * d_slices))
    assert e_feat <= max(TOL, 4 * d_feat) and e_sums <= max(TOL, 4 * d_sums) and e_slices <= max(TOL, 4 * d_slices)
    assert len(only) == 1 and torch.equal(only[0], outs[3])                       # output_blocks=[3] is the last entry, bitwise


def test_inception_runs_f32_in_every_precision_mode(gold, net3):
    from ideas_amd import precision
    x = _case(gold, "up").cuda()
    a = net3(x)[0]
    with precision.activations(BF):
        b = net3(x)[0]
        assert precision.activation_dtype() == BF
    assert b.dtype == torch.float32 and torch.equal(a, b)
    assert precision.activation_dtype() == torch.float32
    xg = x.clone().requires_grad_(True)                                          # no graph is built through the frozen network
    assert not net3(xg)[0].requires_grad
    with pytest.raises(RuntimeError, match=r"\[B, 3, H, W\]"):
        net3(x[:, :2])


# ------------------------------------------------------------------------------------------------- ideas_amd.fid on a generator
@pytest.fixture(scope="module")
def g_ema(gold):
    from ideas_amd.model import Generator
    meta = gold.json("meta")["gen"]
    torch.manual_seed(meta["seed"])
    g = Generator(meta["size"], meta["style_dim"], meta["n_mlp"])
    sums = FR.checksums(g.state_dict())
    for k, (s, a) in meta["checksums"].items():
        assert sums[k][0] == pytest.approx(s, rel=1e-5, abs=1e-5) and sums[k][1] == pytest.approx(a, rel=1e-5), k
    pre = "gen/fill/"
    params = dict(g.named_parameters())
    with torch.no_grad():
        for k in gold.keys():
            if k.startswith(pre):
                params[k[len(pre):]].copy_(gold.t(k))
    assert all(float(p.detach().abs().max()) == 0 for n, p in params.items() if n.endswith("noise.weight"))
    return g.eval().cuda()


def _pinned_randn(monkeypatch, gold, dim):
    """How the draw is pinned: ``extract_feature_from_samples`` draws ``torch.randn(batch, style_dim, device=device)`` once per
    batch; the fixture was made with a ``randn`` that hands out the rows of ``gen/latents`` in order, and so is this one.  (The noise
    images the generator draws itself do not enter: the fixture's noise weights are zero.)"""
    latents = gold.t("gen/latents")
    pos = [0]

    def randn(batch, d, device=None):
        assert d == dim
        r = latents[pos[0]:pos[0] + batch].to(device)
        pos[0] += batch
        return r
    monkeypatch.setattr(torch, "randn", randn)
    return pos


@pytest.mark.parametrize("idx,tag,trunc", [(0, "t100", 1.0), (1, "t70", 0.7)], ids=("t100", "t70"))
def test_extract_feature_from_samples_matches_the_reference(gold, g_ema, net3, monkeypatch, idx, tag, trunc):
    from ideas_amd import fid as FID
    meta = gold.json("meta")["gen"]
    pos = _pinned_randn(monkeypatch, gold, meta["style_dim"])
    mean_latent = gold.t("gen/mean_latent").cuda() if trunc < 1 else None
    feats = FID.extract_feature_from_samples(g_ema, net3, trunc, mean_latent, meta["batch"], meta["n_sample"], "cuda")
    assert pos[0] == meta["n_sample"] == 5 and tuple(feats.shape) == (5, 2048) and feats.device.type == "cpu"     # batches 2, 2, 1
    d = float(gold.z["gen/f32_dev"][idx])
    err = rel_err(feats, gold.t(f"gen/feat_{tag}"))
    print(tag, "rel err", err, "bound", max(TOL, 4 * d))
    assert err <= max(TOL, 4 * d)
    pos[0] = 0                                                                    # a remainder of zero draws nothing and does not crash
    assert tuple(FID.extract_feature_from_samples(g_ema, net3, trunc, mean_latent, 2, 4, "cuda").shape) == (4, 2048) and pos[0] == 4


def test_fid_end_to_end_matches_the_reference(gold, g_ema, net3, monkeypatch):
    """Generator -> Inception -> FeatureStats -> calc_fid between the truncation-1 and the truncation-0.7 samples, on the leading
    four feature dimensions (five samples each: more dimensions would be singular), against the reference's value within 4 x the
    reference's own f32-from-f64 deviation of that number (1.1e-6)."""
    from ideas_amd import fid as FID
    meta = gold.json("meta")["gen"]
    stats = []
    for trunc in (1.0, 0.7):
        pos = _pinned_randn(monkeypatch, gold, meta["style_dim"])
        ml = gold.t("gen/mean_latent").cuda() if trunc < 1 else None
        stats.append(FID.sample_statistics(g_ema, net3, trunc, ml, meta["batch"], meta["n_sample"], "cuda"))
        assert stats[-1].n == 5 and pos[0] == 5
    (ma, ca), (mb, cb) = [(s.mean()[:4], s.cov()[:4, :4]) for s in stats]
    got = float(FID.calc_fid(ma, ca, mb, cb))
    want, dev = float(gold.z["gen/fid4"]), float(gold.z["gen/fid4_dev"])
    err = abs(got - want) / abs(want)
    print("fid4", got, "reference", want, "rel err", err, "bound", max(1e-9, 4 * dev))
    assert err <= max(1e-9, 4 * dev)


# ------------------------------------------------------------------------------------------------- command lines
def test_cli_calc_inception_then_fid(tmp_path):
    """calc_inception.py on a folder of eight 32x32 PNGs, then fid.py with a tiny generator against that pickle: each a fresh child
    process under its own timeout.  (Most of the time is scipy's square root of the 2048 x 2048 product.)"""
    from PIL import Image
    from ideas_amd.model import Generator
    torch.save(FR.backbone_state(), tmp_path / "inception.pth")
    rng = np.random.RandomState(0)
    os.makedirs(tmp_path / "toys")
    for i in range(8):
        Image.fromarray(rng.randint(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / "toys" / f"{i}.png")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "calc_inception.py"), "--size", "32", "--batch", "3", "--n_sample", "7", "--flip",
           "--dataset_type", "normal", "--num_workers", "0", "--inception_weights", str(tmp_path / "inception.pth"), str(tmp_path / "toys")]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "extracted 7 features" in r.stdout
    with open(tmp_path / "inception_toys.pkl", "rb") as f:
        emb = pickle.load(f)
    assert set(emb) == {"mean", "cov", "size", "path"} and emb["size"] == 32 and emb["path"] == str(tmp_path / "toys")
    assert emb["mean"].shape == (2048,) and emb["cov"].shape == (2048, 2048) and np.array_equal(emb["cov"], emb["cov"].T)
    assert np.isfinite(emb["mean"]).all() and np.isfinite(emb["cov"]).all() and float(np.diagonal(emb["cov"]).min()) >= -1e-9

    torch.manual_seed(7)
    torch.save({"g_ema": Generator(32, 32, 2).state_dict()}, tmp_path / "g.pt")
    cmd = [sys.executable, os.path.join(ROOT, "fid.py"), "--size", "32", "--latent", "32", "--n_mlp", "2", "--batch", "4", "--n_sample", "6",
           "--truncation", "0.8", "--truncation_mean", "64", "--inception", str(tmp_path / "inception_toys.pkl"),
           "--inception_weights", str(tmp_path / "inception.pth"), str(tmp_path / "g.pt")]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "extracted 6 features" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("fid:")]
    assert len(line) == 1 and np.isfinite(float(line[0].split()[1]))
