#!/usr/bin/env python3
"""Generate tests/golden/fid.npz: the REFERENCE's own FID Inception-v3 (stylegan2/inception.py), ``calc_fid`` and
``extract_feature_from_samples`` (stylegan2/fid.py), on the CPU, every network quantity in f32 and again in f64.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied: the script imports
its inception.py (``torchvision.models`` is tests/fid_ref.py's seeded stand-in, ``load_state_dict_from_url`` returns the seeded
state), cuts the two functions of fid.py out of its syntax tree, feeds seeded inputs and stores arrays.  The f64 results are stored (as
float32 arrays where they are network outputs); ``*/f32_dev`` is the reference's own f32 run against its f64 run, max-abs over
max-abs -- the input of the tests' tolerances.

* The backbone is NOT stored (95 MB): ``meta["backbone"]`` has the seed, keys / shapes and per-key (sum, abs-sum) checksums.
* ``net/{case}/*`` for the cases of ``fid_ref.CASES`` (B = 2: one smooth and one noise image; 64x48 is upsampled, 299x299 is the
  identity, 320x320 is downsampled, ``norm01`` runs ``normalize_input=True`` on [0, 1] data).  The inputs are NOT stored (the 320x320
  noise image alone is past the size limit): ``fid_ref.case_input`` remakes them from a seed, ``x_sums`` = per-sample (sum, abs-sum)
  guards the remake.  ``feat`` [2, 2048]; ``sums`` [3, 2, 2] = per block 0-2 and sample (sum, abs-sum); ``slice{k}`` = block k at
  ``fid_ref.block_slice`` (the first and the last 16 channels -- the last are the pooled branch of Mixed_6e in block 2 -- at the
  3x3 top-left pixels: a corner, two edges and an interior pixel, so the divisors 4 / 6 / 9 and the unpadded pools are pinned);
  ``f32_dev`` = [feat, sums, slices].
* ``fid/{good,singular}/*``: ``calc_fid`` on seeded statistics.  ``good``: D = 24, n = 400 samples of two different Gaussians;
  ``singular``: a rank-deficient pair, n = 16 < D = 24.  ``sample_mean, sample_cov, real_mean, real_cov`` (f64), ``fid``, ``dev`` =
  the reference's own numerical noise |fid(s, r) - fid(r, s)| / |fid| (the distance is symmetric in exact arithmetic);
  ``meta["fid"][case]`` = the branches the reference took (``retried``: the eps offset, ``complex``: a complex square root).
* ``stats/*``: ``np.mean(F, 0)`` and ``np.cov(F, rowvar=False)`` as fid.py:97-98 computes them from the f32 matrix
  ``fid_ref.stats_features()`` [37, 2048] (remade from its seed; ``stats/f_sums`` guards it).  The 2048 x 2048 covariance is stored as
  its diagonal, its leading 64 x 64 block and (sum, abs-sum); ``*_true`` = the same from an extended-precision (long double)
  evaluation rounded to f64, ``stats/dev`` = [mean, cov] the reference's deviation from it, max-abs over max-abs (the mean is
  accumulated in f32 by numpy, the covariance in f64).
* ``gen/*``: ``extract_feature_from_samples`` on the seeded ``Generator(32, 32, 2)`` of the LPIPS fixture (same seeds, same filled
  biases; the NOISE WEIGHTS ARE SET TO ZERO, so that the noise images the generator draws from the global RNG do not enter),
  ``n_sample = 5``, ``batch_size = 2`` (batches 2, 2 and the remainder 1), at truncation 1 and 0.7.  The function draws
  ``torch.randn(batch, 512)``: its ``torch`` is a stand-in whose ``randn`` hands out ``gen/latents`` [5, 32] in order -- that is how
  the draw is pinned on both sides.  ``gen/mean_latent`` [1, 32] = the truncation latent; ``gen/feat_t{100,70}`` [5, 2048];
  ``gen/f32_dev`` [2]; ``gen/fid4`` = calc_fid between the statistics (np.mean / np.cov) of the leading 4 feature dimensions of the
  two runs, ``gen/fid4_dev`` = the reference's own f32-from-f64 deviation of that number.

    python tests/golden/make_golden_fid.py
"""
import ast
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                      # noqa: E402
import make_golden_stylegan2_gen as MGG       # noqa: E402
import fid_ref as FR                          # noqa: E402

GEN_SEED, FILL_SEED, STYLE_DIM, N_MLP, GEN_SIZE = 630, 631, 32, 2, 32      # the generator of make_golden_lpips.py
LATENT_SEED, FID_SEED = 5100, 5200
N_SAMPLE, BATCH = 5, 2


def import_inception():
    mods = MG.import_reference()
    tv = sys.modules["torchvision"]
    tv.models = FR.as_torchvision_models()
    sys.modules.update({"torchvision.models": tv.models, "torchvision.models.inception": tv.models.inception})
    sys.path.insert(0, os.path.join(MG.REF, "stylegan2"))
    import inception as RI
    RI.load_state_dict_from_url = lambda *a, **k: FR.backbone_state()
    return mods, RI


def dev(a32, a64):
    den = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / (den if den > 0 else 1.0)


def f32(t):
    return MG.npy(t.detach().float())


def run_net(net, x, normalize):
    net.normalize_input = normalize
    with torch.no_grad():
        outs = net(x.to(next(net.parameters()).dtype))
    net.normalize_input = False
    assert len(outs) == 4 and all(bool(torch.isfinite(o).all()) for o in outs)
    return outs


def gen_net(out, net32, net64):
    for tag, (h, w, normalize) in FR.CASES.items():
        x = FR.case_input(tag)
        o64, o32 = run_net(net64, x, normalize), run_net(net32, x, normalize)
        feat64, feat32 = o64[3].reshape(2, -1), o32[3].reshape(2, -1)
        sums = lambda os_: torch.tensor([[[float(o[n].double().sum()), float(o[n].double().abs().sum())] for n in range(2)]
                                         for o in os_[:3]], dtype=torch.float64)
        d = [dev(feat32, feat64), dev(sums(o32), sums(o64)),
             max(dev(FR.block_slice(a), FR.block_slice(b)) for a, b in zip(o32[:3], o64[:3]))]
        out[f"net/{tag}/x_sums"] = np.array([[float(x[n].double().sum()), float(x[n].double().abs().sum())] for n in range(2)])
        out[f"net/{tag}/feat"] = f32(feat64)
        out[f"net/{tag}/sums"] = MG.npy(sums(o64))
        for k in range(3):
            out[f"net/{tag}/slice{k}"] = f32(FR.block_slice(o64[k]))
        out[f"net/{tag}/f32_dev"] = np.array(d, np.float64)
        z = float((feat64 == 0).double().mean())
        print(tag, tuple(x.shape), "blocks", [tuple(o.shape) for o in o64], "feat max %.3f zeros %.3f" % (float(feat64.max()), z),
              "sample diff %.3f" % float((feat64[0] - feat64[1]).abs().max() / feat64.abs().max()), "f32_dev (feat, sums, slices)", d)


def reference_functions():
    """``extract_feature_from_samples`` and ``calc_fid`` of stylegan2/fid.py, compiled on their own (the file imports tqdm, scipy,
    ``model`` and ``calc_inception`` at module level)."""
    from scipy import linalg
    path = os.path.join(MG.REF, "stylegan2", "fid.py")
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("extract_feature_from_samples", "calc_fid")]
    assert len(fns) == 2
    calls = []
    spy = types.SimpleNamespace(sqrtm=lambda *a, **k: (calls.append(1), linalg.sqrtm(*a, **k))[1])
    scope = {"torch": torch, "np": np, "linalg": spy, "tqdm": lambda it: it}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), scope)
    return scope, calls


def gen_calc_fid(out, meta, scope, calls):
    from scipy import linalg
    rng = np.random.default_rng(FID_SEED)
    D = 24
    a, b = rng.normal(size=(D, D)) / np.sqrt(D), rng.normal(size=(D, D)) / np.sqrt(D)
    cases = {"good": (rng.normal(size=(400, D)) @ a + rng.normal(size=D), rng.normal(size=(400, D)) @ b * 1.5 + rng.normal(size=D)),
             "singular": (rng.normal(size=(16, D)) @ a, rng.normal(size=(16, D)) @ b + 0.3)}
    meta["fid"] = {}
    for tag, (fs, fr) in cases.items():
        sm, sc, rm, rc = np.mean(fs, 0), np.cov(fs, rowvar=False), np.mean(fr, 0), np.cov(fr, rowvar=False)
        del calls[:]
        fid = scope["calc_fid"](sm, sc, rm, rc)
        retried = len(calls) == 2
        first, _ = linalg.sqrtm(sc @ rc, disp=False)
        branch = dict(retried=retried, complex=bool(np.iscomplexobj(first)) if not retried else
                      bool(np.iscomplexobj(linalg.sqrtm((sc + np.eye(D) * 1e-6) @ (rc + np.eye(D) * 1e-6)))),
                      rank=[int(np.linalg.matrix_rank(sc)), int(np.linalg.matrix_rank(rc))])
        back = scope["calc_fid"](rm, rc, sm, sc)
        assert np.isfinite(fid) and np.isfinite(back) and not np.iscomplexobj(fid)
        out[f"fid/{tag}/sample_mean"], out[f"fid/{tag}/sample_cov"], out[f"fid/{tag}/real_mean"], out[f"fid/{tag}/real_cov"] = sm, sc, rm, rc
        out[f"fid/{tag}/fid"] = np.array(float(fid))
        out[f"fid/{tag}/dev"] = np.array(abs(float(fid) - float(back)) / abs(float(fid)))
        meta["fid"][tag] = branch
        print("calc_fid", tag, float(fid), "reverse", float(back), "dev", float(out[f"fid/{tag}/dev"]), branch)
    assert not meta["fid"]["good"]["retried"] and meta["fid"]["good"]["rank"] == [D, D], "the good case must take the plain branch"
    assert meta["fid"]["singular"]["rank"][0] < D and meta["fid"]["singular"]["rank"][1] < D
    # the intended branch of the rank-deficient pair: whichever non-plain path the reference's sqrtm leads it to -- the eps retry
    # (a non-finite root) or the complex root whose real part is taken; a plain real finite root would test nothing new
    assert meta["fid"]["singular"]["retried"] or meta["fid"]["singular"]["complex"], "pick another FID_SEED"


def gen_stats(out):
    f = FR.stats_features()
    mean, cov = np.mean(f.numpy(), 0), np.cov(f.numpy(), rowvar=False)           # fid.py:97-98
    assert mean.dtype == np.float32 and cov.dtype == np.float64
    L = f.numpy().astype(np.longdouble)
    mt = L.mean(0)
    c = L - mt
    ct = (c.T @ c / (L.shape[0] - 1)).astype(np.float64)
    mt = mt.astype(np.float64)
    d = [float(np.abs(mean - mt).max() / np.abs(mt).max()), float(np.abs(cov - ct).max() / np.abs(ct).max())]
    out["stats/f_sums"] = np.array([float(f.double().sum()), float(f.double().abs().sum())])
    out["stats/mean"], out["stats/mean_true"] = mean, mt
    for name, m in (("cov", cov), ("cov_true", ct)):
        out[f"stats/{name}_diag"], out[f"stats/{name}_block"] = np.diagonal(m).copy(), m[:64, :64].copy()
        out[f"stats/{name}_sums"] = np.array([m.sum(), np.abs(m).sum()])
    out["stats/dev"] = np.array(d, np.float64)
    print("stats: dev (mean, cov)", d)


def gen_generator(out, meta, RL, RI, scope):
    torch.manual_seed(GEN_SEED)
    g_ema = RL.Generator(GEN_SIZE, STYLE_DIM, N_MLP)
    meta["gen"] = dict(seed=GEN_SEED, fill_seed=FILL_SEED, size=GEN_SIZE, style_dim=STYLE_DIM, n_mlp=N_MLP, n_sample=N_SAMPLE, batch=BATCH,
                       checksums=FR.checksums(g_ema.state_dict()))
    fill = MGG.fill(g_ema, FILL_SEED)
    with torch.no_grad():
        for name, p in g_ema.named_parameters():
            if name.endswith("noise.weight"):
                p.zero_()
                fill[name] = p.detach().clone()
    for name, v in fill.items():
        out[f"gen/fill/{name}"] = f32(v)
    g_ema.eval()
    gen = torch.Generator().manual_seed(LATENT_SEED)
    latents = torch.randn(N_SAMPLE, STYLE_DIM, generator=gen)
    with torch.no_grad():
        mean_latent = g_ema.style(torch.randn(4096, STYLE_DIM, generator=gen)).mean(0, keepdim=True)
    out["gen/latents"], out["gen/mean_latent"] = f32(latents), f32(mean_latent)
    inc32 = RI.InceptionV3([3], normalize_input=False).eval()
    feats, devs = {}, []
    for trunc, tag in ((1.0, "t100"), (0.7, "t70")):
        res = {}
        for dtype in (torch.float64, torch.float32):
            g, inc = copy.deepcopy(g_ema).to(dtype), copy.deepcopy(inc32).to(dtype)
            pos = [0]

            def randn(batch, dim, device=None):
                assert dim == 512                                   # (the reference hard-codes its own generator's latent size)
                r = latents[pos[0]:pos[0] + batch].to(dtype)
                pos[0] += batch
                return r
            scope["torch"] = types.SimpleNamespace(randn=randn, cat=torch.cat, no_grad=torch.no_grad)
            scope["g"] = g                                          # (fid.py:25 calls the module-level ``g``, not its argument)
            res[dtype] = scope["extract_feature_from_samples"](g, inc, trunc, mean_latent.to(dtype) if trunc < 1 else None, BATCH,
                                                               N_SAMPLE, "cpu")
            assert pos[0] == N_SAMPLE and tuple(res[dtype].shape) == (N_SAMPLE, 2048) and bool(torch.isfinite(res[dtype]).all())
        scope["torch"] = torch
        out[f"gen/feat_{tag}"] = f32(res[torch.float64])
        feats[tag] = res
        devs.append(dev(res[torch.float32], res[torch.float64]))
    out["gen/f32_dev"] = np.array(devs, np.float64)
    fids = {}
    for dtype in (torch.float64, torch.float32):
        a, b = feats["t100"][dtype].numpy()[:, :4], feats["t70"][dtype].numpy()[:, :4]
        fids[dtype] = float(scope["calc_fid"](np.mean(a, 0), np.cov(a, rowvar=False), np.mean(b, 0), np.cov(b, rowvar=False)))
    out["gen/fid4"] = np.array(fids[torch.float64])
    out["gen/fid4_dev"] = np.array(abs(fids[torch.float32] - fids[torch.float64]) / abs(fids[torch.float64]))
    print("gen: f32_dev", devs, "fid4", fids[torch.float64], "dev", float(out["gen/fid4_dev"]),
          "t100 vs t70 feature diff %.3f" % float((res[torch.float64] - feats["t100"][torch.float64]).abs().max()))


def main():
    (RM, RU, RL, RO), RI = import_inception()
    net32 = RI.InceptionV3([0, 1, 2, 3], normalize_input=False).eval()
    net64 = copy.deepcopy(net32).double()
    out, meta = {}, {}
    sd = FR.backbone_state()
    ref_vals = [v for k, v in net32.state_dict().items()]
    assert len(sd) == FR.N_ENTRIES and sum(v.numel() for k, v in sd.items() if not k.endswith("num_batches_tracked")
                                            and "running" not in k) == FR.N_PARAMS
    own = [v for k, v in sd.items() if not k.startswith("fc.")]
    assert len(ref_vals) == len(own) and all(torch.equal(a, b) for a, b in zip(ref_vals, own)), "the reference did not load the seeded state"
    meta["backbone"] = dict(seed=FR.BACKBONE_SEED, keys=[[k, list(v.shape)] for k, v in sd.items()], checksums=FR.checksums(sd))
    gen_net(out, net32, net64)
    scope, calls = reference_functions()
    gen_calc_fid(out, meta, scope, calls)
    gen_stats(out)
    gen_generator(out, meta, RL, RI, scope)
    assert all(bool(np.isfinite(v).all()) for v in out.values())
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "fid.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("fid.npz", len(out), "arrays,", size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
