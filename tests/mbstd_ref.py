"""Plain-torch restatement of the minibatch standard deviation of ``stylegan2.model.Discriminator.forward`` (model.py:697-705) and of
the closed forms of its backward and of the backward's backward that csrc/minibatch_stddev.hip evaluates.  Runs in whatever dtype
it is given (the tests use f64).  tests/test_stylegan2_disc.py pins it to the reference's own captured block output."""
import torch


def _split(x, group, feat):
    b, c, h, w = x.shape
    g = min(b, group)
    if b % g or c % feat:
        raise RuntimeError("minibatch_stddev: batch % group or channels % feat")
    return g, b // g, c // feat


def _stats(x, group, feat, eps):
    """u = x - mean_g x and sd, both [G, M, feat, C / feat, H, W] (sd broadcast over G)."""
    b, c, h, w = x.shape
    g, m, cf = _split(x, group, feat)
    v = x.reshape(g, m, feat, cf, h, w)                 # the group index is the outer one
    u = v - v.mean(0, keepdim=True)                     # two-pass: centre first
    sd = (u.square().mean(0, keepdim=True) + eps).sqrt()
    return u, sd


def minibatch_stddev(x, group=4, feat=1, eps=1e-8):
    b, c, h, w = x.shape
    g, m, cf = _split(x, group, feat)
    _, sd = _stats(x, group, feat, eps)
    s = sd[0].mean((2, 3, 4))                           # [M, feat]
    extra = s[None, :, :, None, None].expand(g, m, feat, h, w).reshape(b, feat, h, w)
    return torch.cat([x, extra], 1)


def backward(x, gout, group=4, feat=1, eps=1e-8):
    """gx = gout[:, :C] + a u / sd,  a[m, f] = (sum_{g, h, w} gout[g M + m, C + f, h, w]) / (K G)."""
    b, c, h, w = x.shape
    g, m, cf = _split(x, group, feat)
    u, sd = _stats(x, group, feat, eps)
    a = gout[:, c:].reshape(g, m, feat, h * w).sum((0, 3)) / (cf * h * w * g)
    return gout[:, :c] + (a[None, :, :, None, None, None] * u / sd).reshape(b, c, h, w)


def backward2(x, gout, v, group=4, feat=1, eps=1e-8):
    """(d gout, d x) of ``backward`` for the cotangent v:
    d gout[:, :C] = v;  d gout[n, C + f] = t[n % M, f],  t = (1 / (K G)) sum_{g, c in chunk f, h, w} v u / sd;
    d x = a ((v - mean_g v) / sd - u (sum_g v u) / (G sd^3))."""
    b, c, h, w = x.shape
    g, m, cf = _split(x, group, feat)
    u, sd = _stats(x, group, feat, eps)
    kg = cf * h * w * g
    a = (gout[:, c:].reshape(g, m, feat, h * w).sum((0, 3)) / kg)[None, :, :, None, None, None]
    vv = v.reshape(g, m, feat, cf, h, w)
    t = (vv * u / sd).sum((0, 3, 4, 5)) / kg            # [M, feat]
    dextra = t[None, :, :, None, None].expand(g, m, feat, h, w).reshape(b, feat, h, w)
    dot = (vv * u).sum(0, keepdim=True)
    dx = a * ((vv - vv.mean(0, keepdim=True)) / sd - u * dot / (g * sd ** 3))
    return torch.cat([v, dextra], 1), dx.reshape(b, c, h, w)
