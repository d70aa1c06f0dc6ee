"""Host-side checks of the payload code: the numpy restatement tests/ecc_ref.py against the definitions of DESIGN.md "Payload coding"
(impulse response, free distance, the plan and stride table, error correction up to half the free distance), ``ideas_amd.ecc.Code``
against it, frame / unframe through the reference encode / decode, and the C ABI of csrc/ecc.hip with its argument errors.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ecc_ref as R
from conftest import ROOT

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
NAMES = ("ideas_ecc_encode", "ideas_ecc_soft", "ideas_ecc_viterbi")
PLAN = [("1/2", 28, 8), ("1/2", 256, 120), ("2/3", 256, 160), ("3/4", 256, 184), ("1/2", 2048, 1016), ("3/4", 2048, 1528)]
STRIDES = {28: 11, 29: 10, 100: 37, 256: 97, 2048: 769}


# ------------------------------------------------------------------------------------------------- the code itself
def test_impulse_response():
    pairs = R.mother([1, 0, 0, 0, 0, 0, 0])
    assert ["%d%d" % tuple(p) for p in pairs] == ["11", "10", "11", "11", "00", "01", "11"]


def test_free_distance_is_10():
    """The minimum weight over all nonzero inputs of length <= 8 (first bit 1: the code is time-invariant), terminated."""
    best = min(int(R.mother((1,) + rest + (0,) * R.TAIL).sum()) for n in range(8) for rest in itertools.product((0, 1), repeat=n))
    assert best == 10


@pytest.mark.parametrize("rate,n,k", PLAN)
def test_plan_table(rate, n, k):
    from ideas_amd import ecc
    pl = R.plan(n, rate)
    assert pl["k"] == k and pl["T"] == k + 6 and pl["m"] <= n < R.kept(k + 8 + 6, rate)
    code = ecc.Code(n, rate)
    assert (code.k_bits, code.k_bytes, code.steps, code.coded_bits) == (k, k // 8, k + 6, pl["m"])
    assert (code.stride, code.stride_inv) == (pl["P"], pl["Pinv"]) and code.stride * code.stride_inv % n == 1
    assert code.rate == rate and code.n_bits == n


def test_stride_table_and_kept_counts():
    from ideas_amd import ecc
    for n, p in STRIDES.items():
        assert R.stride(n) == p and ecc.stride_of(n) == p
    for rate in R.RATES:
        for T in range(0, 40):
            assert ecc.kept_outputs(T, rate) == R.kept(T, rate)
    assert [R.kept(6, r) for r in ("1/2", "2/3", "3/4")] == [12, 9, 8]
    assert sorted(ecc.RATES) == sorted(R.RATES) and all(ecc.RATES[r] == R.RATES[r][0] for r in R.RATES)


def test_code_refuses_unknown_rates_and_small_images():
    from ideas_amd import ecc
    with pytest.raises(ValueError, match="rate"):
        ecc.Code(256, "5/6")
    with pytest.raises(ValueError, match="too small"):
        ecc.Code(27, "1/2")
    assert ecc.Code(28, "1/2").k_bits == 8
    with pytest.raises(ValueError):
        R.plan(27, "1/2")


def codeword_soft(info_rows, n, rate, mag=64):
    coded = R.unpack(R.encode(info_rows, n, rate), n)
    return ((coded.astype(np.int32) * 2 - 1) * mag).astype(np.int8)


@pytest.mark.parametrize("rate", sorted(R.RATES))
def test_noiseless_round_trip_with_fill(rate):
    rng = np.random.default_rng(7)
    for n in (28, 29, 100, 256):
        pl = R.plan(n, rate)
        info = rng.integers(0, 256, (3, pl["k"] // 8), dtype=np.uint8)
        fill = R.pack(rng.integers(0, 2, (3, n)))
        coded = R.encode(info, n, rate, fill)
        assert coded.shape == (3, (n + 7) // 8)
        if n % 8:
            assert not (coded[:, -1] & ((1 << (8 - n % 8)) - 1)).any()
        bits, fbits = R.unpack(coded, n), R.unpack(fill, n)
        free = np.ones(n, bool)
        free[R.positions(n, pl["P"], pl["m"])] = False
        assert free.sum() == n - pl["m"] and np.array_equal(bits[:, free], fbits[:, free])
        got, metric = R.decode(((bits.astype(np.int32) * 2 - 1) * 64).astype(np.int8), n, rate)
        assert np.array_equal(got, info) and metric.tolist() == [64 * pl["m"]] * 3


def test_any_four_sign_flips_are_corrected_at_rate_half():
    """d_free = 10: four flips of uniform magnitude 64 leave the sent path ahead of every other by at least 2 * 64 -- no ties."""
    n, rate = 256, "1/2"
    pl = R.plan(n, rate)
    rng = np.random.default_rng(11)
    info = rng.integers(0, 256, (60, pl["k"] // 8), dtype=np.uint8)
    soft = codeword_soft(info, n, rate)
    pos = R.positions(n, pl["P"], pl["m"])
    for b in range(info.shape[0]):
        flips = pos[rng.choice(pl["m"], 4, replace=False)]
        if b < 20:                                            # a burst in the codeword: four consecutive kept outputs
            s = int(rng.integers(0, pl["m"] - 4))
            flips = pos[s:s + 4]
        soft[b, flips] = -soft[b, flips]
    got, metric = R.decode(soft, n, rate)
    assert np.array_equal(got, info)
    assert metric.tolist() == [64 * (pl["m"] - 8)] * info.shape[0]


def test_frame_and_unframe_compose_with_the_reference_code():
    from ideas_amd import ecc, stego
    n, rate = 256, "2/3"
    code = ecc.Code(n, rate)
    payload = bytes(range(97))
    rows = stego.frame(payload, code.k_bytes, torch.Generator().manual_seed(2)).numpy()
    assert rows.shape == (-(-(8 + 97) // code.k_bytes), code.k_bytes)
    soft = codeword_soft(rows, n, rate, mag=20)
    got, _ = R.decode(soft, n, rate)
    assert stego.unframe(got) == payload
    soft[0, :40] = 0                                          # erasures the code fills in
    assert stego.unframe(R.decode(soft, n, rate)[0]) == payload
    with pytest.raises(stego.PayloadError):
        stego.unframe(R.decode(-soft, n, rate)[0])


def test_soft_reference_by_hand():
    z = np.array([[-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0, np.nan]], np.float32)
    assert R.soft(z, 1).tolist() == [[-127, -127, -64, 0, 32, 64, 127, 127, -127]]
    assert R.soft(z, 1, gain=7.5).tolist() == [[-15, -15, -8, 0, 4, 8, 15, 15, -15]]
    s2 = R.soft(np.array([[-0.75, -0.25, 0.25, 0.75, 0.0, -0.5]], np.float32), 2, gain=8.0)
    # centres -0.75 (00), -0.25 (01), 0.25 (10), 0.75 (11); at a centre the nearest other value of a bit is 1 or 2 steps away
    assert s2.reshape(-1, 2).tolist() == [[-32, -8], [-8, 8], [8, -8], [32, 8], [0, 0], [-16, 0]]


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_exports_and_binds_the_three_entry_points():
    from ideas_amd import _lib, op
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    mk = open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()
    assert "ecc.hip" in mk and "ecc.usage.txt" in mk
    for name in ("ecc_encode", "ecc_soft", "ecc_viterbi"):
        assert callable(getattr(op, name)) and name in op.__all__
    for rate, (rid, _, _, _) in R.RATES.items():
        assert re.search(r"#define\s+IDEAS_ECC_RATE_%s\s+%d\b" % (rate.replace("/", "_"), rid), hdr)


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def enc(coded=a, info=a, fill=a, B=1, n=256, k=120, rate=0, P=97, Pinv=pow(97, -1, 256)):
        return lib.ideas_ecc_encode(coded, info, fill, B, n, k, rate, P, Pinv, None)
    assert enc(coded=None) == E_NULL and enc(info=None) == E_NULL
    assert enc(B=0) == E_SHAPE and enc(n=0) == E_SHAPE and enc(k=0) == E_SHAPE and enc(k=-8) == E_SHAPE
    assert enc(k=116) == E_SHAPE                                                  # k % 8
    assert enc(k=128) == E_SHAPE                                                  # m(134) = 268 > 256
    assert enc(P=96) == E_SHAPE and enc(P=0) == E_SHAPE and enc(P=256 + 97) == E_SHAPE      # gcd(96, 256) = 32; outside [1, n)
    assert enc(Pinv=pow(97, -1, 256) + 2) == E_SHAPE and enc(Pinv=0) == E_SHAPE
    assert enc(rate=3) == E_UNSUPPORTED and enc(rate=-1) == E_UNSUPPORTED
    assert enc(fill=None, B=0) == E_SHAPE                                         # NULL fill is fine: the next check answers

    def soft(out=a, z=a, B=1, L=37, sigma=2, gain=64.0, dtype=_lib.F32):
        return lib.ideas_ecc_soft(out, z, B, L, sigma, gain, dtype, None)
    assert soft(out=None) == E_NULL and soft(z=None) == E_NULL
    assert soft(B=0) == E_SHAPE and soft(L=-1) == E_SHAPE
    assert soft(sigma=0) == E_UNSUPPORTED and soft(sigma=9) == E_UNSUPPORTED
    assert soft(dtype=_lib.F16) == E_UNSUPPORTED and soft(dtype=_lib.F32_B3) == E_UNSUPPORTED
    assert soft(gain=0.0) == E_UNSUPPORTED and soft(gain=-1.0) == E_UNSUPPORTED and soft(gain=float("inf")) == E_UNSUPPORTED
    assert soft(gain=float("nan")) == E_UNSUPPORTED

    def vit(info=a, metric=a, soft=a, ws=a, B=1, n=256, k=120, rate=0, P=97):
        return lib.ideas_ecc_viterbi(info, metric, soft, ws, B, n, k, rate, P, None)
    assert vit(info=None) == E_NULL and vit(soft=None) == E_NULL
    assert vit(B=0) == E_SHAPE and vit(k=116) == E_SHAPE and vit(k=128) == E_SHAPE and vit(P=96) == E_SHAPE
    assert vit(rate=7) == E_UNSUPPORTED
    assert vit(metric=None, ws=None, B=0) == E_SHAPE                              # both optional
    big = 1 << 20                                                                 # T = k + 6 above 2^20, whatever the room
    assert vit(n=1 << 30, k=big, P=3) == E_SHAPE and vit(n=1 << 30, k=big, P=3, ws=None) == E_SHAPE
    assert vit(n=1 << 30, k=big - 8, P=0) == E_SHAPE                              # (T = 2^20 - 2 is allowed: the stride answers)
    # survivors above the LDS size need a workspace: T = 4102 > 4096
    assert vit(n=8204, k=4096, P=R.stride(8204), ws=None) == E_UNSUPPORTED
    assert vit(n=8204, k=4096, P=0, ws=None) == E_SHAPE


def test_ops_refuse_host_tensors():
    from ideas_amd import ecc, op
    code = ecc.Code(256, "1/2")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.ecc_encode(torch.zeros(1, 15, dtype=torch.uint8), 256, 120, 0, 97, pow(97, -1, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.ecc_soft(torch.zeros(1, 8), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ecc.decode(code, torch.zeros(1, 256, dtype=torch.int8))


def test_command_lines_accept_ecc(capsys):
    import evaluate
    import extract
    import hide
    for mod in (hide, extract, evaluate):
        with pytest.raises(SystemExit) as e:
            mod.main(["--help"])
        assert e.value.code == 0 and "--ecc" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:                      # a bad rate is a usage error, before anything is loaded
        evaluate.main(["--ecc", "5/6", "nowhere.pt"])
    assert e.value.code == 2 and "5/6" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        hide.main(["--ckpt", "nowhere.pt", "--payload", "p", "--out", "o", "--ecc", "1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        extract.main(["--ckpt", "nowhere.pt", "--out", "o", "--ecc", "half", "x.png"])
    assert e.value.code == 2
