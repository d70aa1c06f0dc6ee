"""The f16 / f64 dtypes of the two drop-in ops at the C ABI (no GPU: every call here returns before a launch)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(name):
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", hdr)
    assert m, f"{name} not declared in ideas_hip.h"
    return int(m.group(1))


@pytest.fixture(scope="module")
def lib():
    from ideas_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libideas_hip.so first (__graft_entry__.build())"
    return _lib.load()


def test_dtype_enum_matches_header():
    from ideas_amd import _lib
    assert _lib.F16 == _header_enum("IDEAS_F16") == 3
    assert _lib.F64 == _header_enum("IDEAS_F64") == 4
    assert (_lib.F32, _lib.BF16) == (_header_enum("IDEAS_F32"), _header_enum("IDEAS_BF16"))


def test_op_dtype_maps_the_four_dtypes_and_act_dtype_stays_narrow():
    from ideas_amd import _lib
    assert _lib.op_dtype(torch.zeros(1, dtype=torch.float16)) == _lib.F16
    assert _lib.op_dtype(torch.zeros(1, dtype=torch.float64)) == _lib.F64
    assert _lib.op_dtype(torch.zeros(1)) == _lib.F32
    assert _lib.op_dtype(torch.zeros(1, dtype=torch.bfloat16)) == _lib.BF16
    with pytest.raises(RuntimeError):
        _lib.op_dtype(torch.zeros(1, dtype=torch.int32))
    for dt in (torch.float16, torch.float64):          # convolutions keep refusing them
        with pytest.raises(RuntimeError):
            _lib.act_dtype(torch.zeros(1, dtype=dt))


@pytest.mark.parametrize("dtype", [3, 4])
@pytest.mark.parametrize("layout", [0, 1])
def test_fused_bias_act_accepts_f16_f64(lib, dtype, layout):
    # NULL x / y: validation reaches the pointer check (-1) instead of refusing the dtype (-3)
    rc = lib.ideas_fused_bias_act(None, None, None, None, None, 64, 4, 16, layout, 3, 0, 0.2, 1.5, dtype, None)
    assert rc == -1, rc


@pytest.mark.parametrize("dtype", [3, 4])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("k", [4, 9, 32])
def test_upfirdn2d_accepts_f16_f64_and_any_fir(lib, dtype, layout, k):
    rc = lib.ideas_upfirdn2d(None, None, None, 1, 4, 16, 16, 16, 16, k, k, 1, 1, 1, 1, 0, 0, 1.0, 1, layout, dtype, None)
    assert rc == -1, rc


def test_large_fir_passes_validation_for_f32_and_bf16(lib):
    x = ctypes.c_void_p(16)        # never dereferenced: the shape check below fails first
    for dtype in (0, 2):
        rc = lib.ideas_upfirdn2d(x, x, x, 0, 4, 16, 16, 16, 16, 12, 12, 1, 1, 1, 1, 0, 0, 1.0, 1, 1, dtype, None)
        assert rc == -2, (dtype, rc)          # IDEAS_E_SHAPE (B = 0), no longer IDEAS_E_UNSUPPORTED for kh > 8


def test_other_entry_points_still_refuse_f16_f64(lib):
    for dtype in (3, 4):
        rc = lib.ideas_blur_fused(None, None, None, 1, 4, 8, 8, 5, 5, 0, 0, 1.0, 1, 1, None, None, None, 0.2, 1.0, dtype, None)
        assert rc == -3, rc
        r = ctypes.c_void_p(16)
        rc = lib.ideas_fir_up2_add(r, r, r, r, 1, 8, 8, 8, 16, 16, 1, 1, 1.0, 1, dtype, None)
        assert rc == -3, rc
        rc = lib.ideas_channel_sum(r, r, 64, 4, 1, dtype, None)
        assert rc == -3, rc
