"""FID, host side (no GPU): the rectangular-padding geometry of the conv family, ``calc_fid`` against the reference's recorded
values (tests/golden/fid.npz, written by tests/golden/make_golden_fid.py from the reference's own fid.py), the state dict of
``ideas_amd.inception.InceptionV3`` against the torchvision stand-in, and the BatchNorm folding.

Tolerance of ``calc_fid``: ``max(1e-9, 4 x the stored deviation)`` relative, the deviation being the reference's own numerical noise
|fid(s, r) - fid(r, s)| / |fid| (2.3e-16 for the well-conditioned pair, 2.6e-9 for the rank-deficient one): the same scipy on the
same f64 inputs should agree near rounding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, Golden
import fid_ref as FR


@pytest.fixture(scope="module")
def gold():
    return Golden("fid.npz")


# ------------------------------------------------------------------------------------------------- ConvGeom.pad_w
RECT = [((1, 7), (0, 3)), ((7, 1), (3, 0)), ((1, 3), (0, 1)), ((3, 1), (1, 0)), ((5, 5), (2, 2))]


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("kernel,padding", RECT, ids=lambda v: "x".join(map(str, v)))
def test_conv_geom_pad_w_matches_f_conv2d(kernel, padding, stride):
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    kh, kw = kernel
    ph, pw = padding
    g = ConvGeom(kh, kw, stride, ph, False, pw)
    for ih, iw in ((9, 11), (8, 8), (17, 17), (7, 12)):
        x, w = torch.zeros(2, 16, ih, iw), torch.zeros(24, 16, kh, kw)
        ref = F.conv2d(x, w, stride=stride, padding=padding)
        assert g.out_size(ih, iw) == tuple(ref.shape[2:])
        L = plan_fwd(tuple(x.shape), w, g)
        assert (L.B, L.Cin, L.IH, L.IW, L.Cout) == (2, 16, ih, iw, 24)
        assert (L.YH, L.YW) == (L.OH, L.OW) == tuple(ref.shape[2:])
        assert (L.TY, L.TX, L.sy, L.sx, L.dy, L.dx) == (kh, kw, stride, stride, 1, 1)
        assert (L.offy, L.offx) == (-ph, -pw) and L.reflect == 0
        assert (L.osy, L.osx, L.ooy, L.oox) == (1, 1, 0, 0)
        assert tuple(L.wview.shape) == (24, kh, kw, 16)
    assert g.rect == (ph != pw) and g.pw == pw


def test_conv_geom_pad_w_none_is_todays_geometry():
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    old = ConvGeom(3, 3, 2, 1, True)                       # the existing positional constructions keep their meaning
    assert (old.kh, old.kw, old.stride, old.pad, old.reflect, old.pad_w) == (3, 3, 2, 1, True, None)
    assert old == ConvGeom(3, 3, 2, 1, True, None) == ConvGeom(3, 3, 2, 1, True, 1) and hash(old) == hash(ConvGeom(3, 3, 2, 1, True, 1))
    assert not old.rect and old.pw == 1
    assert ConvGeom(3, 3, 1, 1) != ConvGeom(3, 3, 1, 1, False, 0)
    w = torch.zeros(8, 4, 3, 3)
    a, b = plan_fwd((1, 4, 9, 7), w, ConvGeom(3, 3, 1, 1)), plan_fwd((1, 4, 9, 7), w, ConvGeom(3, 3, 1, 1, False, 1))
    for f in ("B", "IH", "IW", "Cin", "YH", "YW", "Cout", "OH", "OW", "TY", "TX", "sy", "sx", "dy", "dx", "offy", "offx", "reflect"):
        assert getattr(a, f) == getattr(b, f), f
    assert (a.offy, a.offx) == (-1, -1)


def test_rectangular_padding_takes_no_specialised_plan():
    """Winograd, the gradient plans, the transposed size and mirror padding all require pad_w == pad."""
    from ideas_amd.op import conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad, plan_fwd, plan_wgrad
    g = ConvGeom(3, 3, 1, 1, False, 0)
    assert g.rect and not CV._wino_ok(g, 8, 16, fwd=False) and not CV._b3_wino_ok(g, 16, 16, 16)
    assert CV._wino_ok(ConvGeom(3, 3, 1, 1), 8, 16, fwd=False) or not CV.WINOGRAD
    w = torch.zeros(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="forward-only"):
        plan_dgrad((1, 8, 9, 7), w, g, (9, 9))
    with pytest.raises(RuntimeError, match="forward-only"):
        plan_wgrad((1, 4, 9, 9), (1, 8, 9, 7), g)
    with pytest.raises(RuntimeError, match="one padding"):
        convT_out_size(4, 4, g)
    with pytest.raises(RuntimeError, match="one padding"):
        plan_fwd((1, 4, 9, 9), w, ConvGeom(3, 3, 1, 1, True, 0))
    # the op front end: a pair is accepted, a gradient through ph != pw is refused before any device work
    x = torch.zeros(1, 4, 9, 9, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        CV._geom(w, 1, (1, 0), False, x, w)
    assert CV._geom(w, 1, (1, 1), False, x, w) == ConvGeom(3, 3, 1, 1)
    with torch.no_grad():
        assert CV._geom(w, 1, (1, 0), False, x, w) == g
    with pytest.raises(RuntimeError, match="pair"):
        CV._geom(w, 1, (1, 0, 1), False)


# ------------------------------------------------------------------------------------------------- calc_fid
def _fid_args(gold, tag):
    return [np.array(gold.z[f"fid/{tag}/{k}"]) for k in ("sample_mean", "sample_cov", "real_mean", "real_cov")]


@pytest.mark.parametrize("tag", ("good", "singular"))
def test_calc_fid_matches_the_reference(gold, tag):
    from ideas_amd.fid import calc_fid
    branch = gold.json("meta")["fid"][tag]
    if tag == "good":
        assert not branch["retried"] and not branch["complex"] and branch["rank"] == [24, 24]
    else:                   # rank 15 < 24: scipy's root of the singular product is complex, the reference keeps its real part
        assert max(branch["rank"]) < 24 and (branch["retried"] or branch["complex"])
    want, dev = float(gold.z[f"fid/{tag}/fid"]), float(gold.z[f"fid/{tag}/dev"])
    got = calc_fid(*_fid_args(gold, tag))
    err = abs(float(got) - want) / abs(want)
    print(tag, "fid", float(got), "reference", want, "rel err", err, "bound", max(1e-9, 4 * dev))
    assert not np.iscomplexobj(got) and err <= max(1e-9, 4 * dev)


def test_calc_fid_retries_a_non_finite_root_with_eps(monkeypatch, capsys):
    """The singular branch itself: a square root with a non-finite entry is taken again on the eps-shifted matrices."""
    from ideas_amd import fid as FID
    seen = []

    def fake(a):
        seen.append(a.copy())
        return np.full_like(a, np.nan) if len(seen) == 1 else np.eye(a.shape[0])
    monkeypatch.setattr(FID, "_sqrtm", fake)
    c = np.diag([1.0, 2.0])
    got = FID.calc_fid(np.zeros(2), c, np.ones(2), 2 * c, eps=1e-3)
    assert len(seen) == 2 and np.array_equal(seen[0], c @ (2 * c)) and np.array_equal(seen[1], (c + 1e-3 * np.eye(2)) @ (2 * c + 1e-3 * np.eye(2)))
    assert got == pytest.approx(2.0 + 3.0 + 6.0 - 2 * 2.0)
    assert "singular" in capsys.readouterr().out


def test_calc_fid_raises_on_a_complex_root():
    """cov_s cov_r = diag(1, -1) has the square root diag(1, i): an imaginary diagonal far above atol = 1e-3."""
    from ideas_amd.fid import calc_fid
    with pytest.raises(ValueError, match="Imaginary component"):
        calc_fid(np.zeros(2), np.diag([1.0, 1.0]), np.zeros(2), np.diag([1.0, -1.0]))


# ------------------------------------------------------------------------------------------------- InceptionV3 (host side)
def test_inception_state_dict_is_torchvisions(gold):
    from ideas_amd.inception import FID_WEIGHTS_FILE, InceptionV3
    sd = FR.backbone_state()
    meta = gold.json("meta")["backbone"]
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["keys"] and len(sd) == FR.N_ENTRIES == 566
    net = InceptionV3([3], weights=sd)
    own = net.state_dict()
    assert list(own) == list(sd) and all(own[k].shape == sd[k].shape and own[k].dtype == sd[k].dtype for k in sd)
    assert all(torch.equal(own[k], sd[k]) for k in sd)                                   # strict=True loaded every entry
    assert sum(p.numel() for p in net.parameters()) == FR.N_PARAMS == 23_850_960
    assert not any(p.requires_grad for p in net.parameters()) and not net.training
    assert InceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3} and InceptionV3.DEFAULT_BLOCK_INDEX == 3
    assert net.output_blocks == [3] and net.last_needed_block == 3
    assert InceptionV3([2, 0], weights=sd).output_blocks == [0, 2]
    with pytest.raises(RuntimeError, match=re.escape(FID_WEIGHTS_FILE)):
        InceptionV3()
    with pytest.raises(NotImplementedError):
        InceptionV3(weights=sd, use_fid_inception=False)
    with pytest.raises(NotImplementedError):
        InceptionV3(weights=sd, requires_grad=True)
    bad = dict(sd)
    del bad["fc.bias"]
    with pytest.raises(RuntimeError):
        InceptionV3(weights=bad)


def test_bn_folding_is_bn_of_conv_in_f64():
    """One (1x7, pad (0, 3)) layer of the seeded stand-in: relu(conv(x, w') + b') against relu(bn(conv(x, w))) in f64."""
    from ideas_amd.inception import BasicConv2d, fold_bn
    ref = FR.seed_(FR.BasicConv2d(16, 24, kernel_size=(1, 7), padding=(0, 3)), 11).double().eval()
    x = torch.randn(2, 16, 6, 9, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    with torch.no_grad():
        want = ref(x)
        w, b = fold_bn(ref.conv.weight, ref.bn.weight, ref.bn.bias, ref.bn.running_mean, ref.bn.running_var, ref.bn.eps)
        got = F.relu(F.conv2d(x, w, b, padding=(0, 3)))
    assert w.dtype == b.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # the module: folded once, cached, remade when a statistic changes in place (what load_state_dict does)
    m = BasicConv2d(16, 24, (1, 7), padding=(0, 3))
    m.load_state_dict(ref.float().state_dict())
    w1, b1 = m.folded()
    assert w1.dtype == torch.float32 and w1.is_contiguous(memory_format=torch.channels_last) and torch.equal(w1, w.float())
    assert m.folded()[0] is w1
    with torch.no_grad():
        m.bn.running_var.mul_(4.0)
    w2, _ = m.folded()
    assert w2 is not w1 and not torch.equal(w2, w1)


def test_c_abi_declares_and_exports_the_fid_kernels():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ideas_pool3x3_fwd", "ideas_global_avg_pool", "ideas_feature_stats_accum"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    for macro, val in (("IDEAS_POOL_MAX_S2", _lib.POOL_MAX_S2), ("IDEAS_POOL_MAX_S1P1", _lib.POOL_MAX_S1P1),
                       ("IDEAS_POOL_AVG_S1P1_VALID", _lib.POOL_AVG_S1P1_VALID), ("IDEAS_FEATURE_STATS_MAX_DIM", _lib.FEATURE_STATS_MAX_DIM)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, hdr).group(1)) == val


def test_pools_and_stats_fail_loudly_without_a_device():
    from ideas_amd.fid import FeatureStats
    from ideas_amd.op import pool as P
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.pool3x3(torch.zeros(1, 4, 5, 5), P.MAX_S2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.global_avg_pool(torch.zeros(1, 4, 5, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FeatureStats(4).update(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="smaller than the 3x3 window"):
        P.pool3x3(torch.zeros(1, 4, 2, 5), P.MAX_S2)
    with pytest.raises(RuntimeError, match="dim must be"):
        FeatureStats(4097)


# ------------------------------------------------------------------------------------------------- MultiResolutionDataset
def test_multi_resolution_dataset_against_the_api_standin(tmp_path, monkeypatch):
    """stylegan2's own LMDB layout (``length``, ``<resolution>-<index:05d>``) through the stand-in of the ``lmdb`` API (the image has
    no ``lmdb``), as tests/test_data.py runs ``LMDBDataset``: the stored PNGs come back bit for bit, at the asked resolution only."""
    import io
    import sys
    from PIL import Image
    import lmdb_standin
    from ideas_amd import data as D
    monkeypatch.setitem(sys.modules, "lmdb", lmdb_standin)
    rng = np.random.RandomState(3)
    arrs = {r: [rng.randint(0, 256, (r, r, 3), dtype=np.uint8) for _ in range(3)] for r in (8, 16)}

    def png(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="png")
        return buf.getvalue()
    items = [(b"length", b"3")] + [(f"{r}-{i:05d}".encode(), png(a)) for r, v in arrs.items() for i, a in enumerate(v)]
    items.append((b"4-00000", png(arrs[8][0])))                                   # an entry whose image is not the size its key says
    lmdb_standin.write_store(str(tmp_path / "db"), items)
    for r in (8, 16):
        ds = D.set_dataset("multires", str(tmp_path / "db"), r)
        assert isinstance(ds, D.MultiResolutionDataset) and len(ds) == 3
        for i in range(3):
            item = ds[i]
            assert item.dtype == torch.uint8 and tuple(item.shape) == (r, r, 3) and np.array_equal(item.numpy(), arrs[r][i])
    assert len(D.MultiResolutionDataset(str(tmp_path / "db"), 8, max_num=2)) == 2
    with pytest.raises(KeyError, match="32-00001"):
        D.MultiResolutionDataset(str(tmp_path / "db"), 32)[1]
    with pytest.raises(ValueError, match="not 4x4"):
        D.MultiResolutionDataset(str(tmp_path / "db"), 4)[0]
    lmdb_standin.write_store(str(tmp_path / "plain"), [(b"00000", png(arrs[8][0]))])
    with pytest.raises(IOError, match="length"):
        D.MultiResolutionDataset(str(tmp_path / "plain"), 8)
