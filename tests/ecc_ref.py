"""The payload code of DESIGN.md "Payload coding" restated in numpy: the mother code (K = 7, 171 / 133 octal), termination, puncturing,
the plan and the interleaver, the float32 soft demapper, and an integer Viterbi decoder vectorised over the 64 states (and the batch)
with the tie rule "on equal metrics b = 0 wins".  The kernels of csrc/ecc.hip must agree with it to the bit."""
import math

import numpy as np

G = (0o171, 0o133)
TAIL = 6
# rate -> (id of include/ideas_hip.h, period, mask of c0, mask of c1), the masks in order of t
RATES = {"1/2": (0, 1, (1,), (1,)), "2/3": (1, 2, (1, 1), (1, 0)), "3/4": (2, 3, (1, 1, 0), (1, 0, 1))}


def parity(x):
    return bin(int(x)).count("1") & 1


def mother(u):
    """Input bits -> [len(u), 2] output pairs (c0, c1), from the zero state, no termination added."""
    r, out = 0, []
    for b in u:
        r = (int(b) << 6) | (r >> 1)
        out.append((parity(r & G[0]), parity(r & G[1])))
    return np.array(out, np.uint8).reshape(-1, 2)


def keep_mask(T, rate):
    """bool [T, 2]: which outputs of which step are kept."""
    _, period, m0, m1 = RATES[rate]
    t = np.arange(T) % period
    return np.stack((np.array(m0, bool)[t], np.array(m1, bool)[t]), 1)


def kept(T, rate):
    return int(keep_mask(T, rate).sum())


def stride(n):
    p = max(1, 3 * n // 8)
    while math.gcd(p, n) != 1:
        p += 1
    return p


def plan(n, rate):
    """-> dict(k, T, m, P, Pinv) for an image of n message bits; ValueError when not even k = 8 fits."""
    if rate not in RATES:
        raise ValueError(f"unknown rate {rate!r}")
    k = 0
    while kept(k + 8 + TAIL, rate) <= n:
        k += 8
    if k < 8:
        raise ValueError(f"n = {n} is too small for rate {rate}")
    P = stride(n)
    return {"k": k, "T": k + TAIL, "m": kept(k + TAIL, rate), "P": P, "Pinv": pow(P, -1, n)}


def positions(n, P, count):
    """Message-bit position of the coded positions 0 .. count - 1."""
    return (np.arange(count, dtype=np.int64) * P) % n


def unpack(rows, nbits):
    return np.unpackbits(np.asarray(rows, np.uint8), axis=1)[:, :nbits]


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=1)          # most significant bit first, pad bits zero


def encode(info_rows, n, rate, fill_rows=None, k=None, P=None):
    """Packed info rows [B, k / 8] -> packed coded rows [B, ceil(n / 8)]."""
    pl = plan(n, rate)
    k = pl["k"] if k is None else k
    P = pl["P"] if P is None else P
    T = k + TAIL
    info = unpack(info_rows, k)
    assert info.shape[1] == k
    msg = np.zeros((info.shape[0], n), np.uint8) if fill_rows is None else unpack(fill_rows, n).copy()
    keep = keep_mask(T, rate).reshape(-1)
    m = int(keep.sum())
    pos = positions(n, P, m)                                        # every other message bit j keeps bit j of the fill (or 0)
    for b in range(info.shape[0]):
        msg[b, pos] = mother(np.concatenate((info[b], np.zeros(TAIL, np.uint8)))).reshape(-1)[keep]
    return pack(msg)


def soft(z, sigma, gain=64.0):
    """z float32 [B, L] -> int8 [B, L * sigma], one float32 operation a step."""
    z = np.asarray(z, np.float32)
    f = np.float32
    step = f(2.0) / f(1 << sigma)
    c = np.where(np.isnan(z), f(-1.0), np.minimum(np.maximum(z, f(-1.0)), f(1.0))).astype(np.float32)
    v = np.arange(1 << sigma)
    cv = (step * (v.astype(np.float32) + f(0.5)) - f(1.0)).astype(np.float32)
    d = (c[..., None] - cv).astype(np.float32)
    d = (d * d).astype(np.float32)                                  # [B, L, 2^sigma]
    out = np.empty(z.shape + (sigma,), np.int8)
    with np.errstate(invalid="ignore"):
        for i in range(sigma):
            one = ((v >> (sigma - 1 - i)) & 1).astype(bool)
            d0, d1 = d[..., ~one].min(-1), d[..., one].min(-1)
            t = (d0 - d1).astype(np.float32)
            t = (t / (step * step)).astype(np.float32)
            t = (t * f(gain)).astype(np.float32)
            out[..., i] = np.clip(np.rint(t), -127, 127).astype(np.int8)
    return out.reshape(z.shape[0], -1)


_S = np.arange(64)
_P0, _P1 = (_S & 31) << 1, ((_S & 31) << 1) | 1
# sign (+1: the output is 1) of output o on the transition into state s with survivor bit b: r = (s << 1) | b
_SIGN = np.array([[[2 * parity(((s << 1) | b) & G[o]) - 1 for s in range(64)] for o in range(2)] for b in range(2)], np.int32)


def viterbi(soft_rows, n, k, rate, P):
    """int8 [B, n] -> (packed info rows [B, k / 8], int32 [B]: the final metric of state 0)."""
    q = np.asarray(soft_rows).astype(np.int32)
    B, T = q.shape[0], k + TAIL
    keep = keep_mask(T, rate)
    m = int(keep.sum())
    assert m <= n and q.shape[1] == n
    dep = np.zeros((B, T * 2), np.int32)
    dep[:, np.flatnonzero(keep.reshape(-1))] = q[:, positions(n, P, m)]
    dep = dep.reshape(B, T, 2)
    pm = np.full((B, 64), -(1 << 30), np.int32)
    pm[:, 0] = 0
    surv = np.empty((T, B, 64), bool)
    for t in range(T):
        q0, q1 = dep[:, t, 0:1], dep[:, t, 1:2]
        m0 = pm[:, _P0] + (_SIGN[0, 0] * q0 + _SIGN[0, 1] * q1)
        m1 = pm[:, _P1] + (_SIGN[1, 0] * q0 + _SIGN[1, 1] * q1)
        dec = m1 > m0                                               # equal: b = 0 wins
        surv[t] = dec
        pm = np.where(dec, m1, m0).astype(np.int32)
    s = np.zeros(B, np.int64)
    u = np.empty((B, T), np.uint8)
    rows = np.arange(B)
    for t in range(T - 1, -1, -1):
        u[:, t] = s >> 5
        s = ((s & 31) << 1) | surv[t, rows, s]
    return pack(u[:, :k]), pm[:, 0].copy()


def decode(soft_rows, n, rate):
    pl = plan(n, rate)
    return viterbi(soft_rows, n, pl["k"], rate, pl["P"])
