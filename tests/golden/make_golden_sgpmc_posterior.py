"""Exact posterior moments of the SGPMC target (targets.SgpmcTarget) on the d = 1 fixture -- run from the repo root:

    python tests/golden/make_golden_sgpmc_posterior.py      # -> tests/golden/posterior_sgpmc_d1_tiny.npz

The recipe of make_golden_posterior.py.  The SGPMC density F(v, theta) is Gaussian in the whitened inducing values v at fixed theta
(precision B = I + W / s2, mode m = B^-1 u / s2), and integrated over v it is the collapsed VFE bound at theta with the same jitter.
So for d = 1 the marginal posterior of the three unconstrained hyper-parameters x = (x_var, x_ls, x_noise),

    logp(x) = F_VFE(theta(x)) + sum over {variance, lengthscale, noise variance} of [log Gamma(c; 2, 1) + log sigmoid(x)],
    variance = softplus(x_var), lengthscale = softplus(x_ls), noise variance = 1e-6 + softplus(x_noise), jitter 1e-5,

can be INTEGRATED by tensor-product Gauss-Legendre quadrature, and with it E[v] = E_x[m(theta(x))] and
Var[v_k] = E_x[(B^-1)_kk + m_k^2] - E[v_k]^2: numbers no sampler produced.  The same checks as make_golden_posterior.py run before
anything is written (box faces, 72 against 112 nodes, the box widened by 25 %).

Stored: X, y, Z of the fixture, jitter, the box, log evidence, mean[3], cov[3,3], m3, m4 per axis (unconstrained x), v_mean[M],
v_var[M], and the log-density at one stated point (x_spot, logp_spot) for the test's spot check.  Nothing outside the repository is read.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.dirname(os.path.abspath(__file__))
JITTER = 1e-5        # gpflow.config.set_default_jitter(1e-5), reference models/sgp_hmc.py:20
NOISE_FLOOR = 1e-6


def logp_batch(x, X, y, Z, want_v=False):
    """The marginal log-density at B points x (B x 3), torch fp64 batched LAPACK, in the whitened op order (A = L^-1 K_uf,
    B = I + A A^T / s2).  want_v: also (m, diag B^-1) per point.  A failed factorization gives -inf."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64))
    sp = torch.nn.functional.softplus
    sf2, ls, s2 = sp(xt[:, 0]), sp(xt[:, 1]), NOISE_FLOOR + sp(xt[:, 2])
    xs, z, yt = torch.as_tensor(X[:, 0]), torch.as_tensor(Z[:, 0]), torch.as_tensor(y)
    N, M = xs.numel(), z.numel()
    eye = torch.eye(M, dtype=torch.float64)
    r2uu = ((z[:, None] - z[None, :]) ** 2)[None] / (ls * ls)[:, None, None]
    r2uf = ((z[:, None] - xs[None, :]) ** 2)[None] / (ls * ls)[:, None, None]
    Kuu = sf2[:, None, None] * torch.exp(-0.5 * r2uu) + JITTER * eye
    Kuf = sf2[:, None, None] * torch.exp(-0.5 * r2uf)
    Luu, info1 = torch.linalg.cholesky_ex(Kuu)
    A = torch.linalg.solve_triangular(Luu, Kuf, upper=False)
    trace = (N * sf2 - (A * A).sum((1, 2))) / (2.0 * s2)
    LB, info2 = torch.linalg.cholesky_ex(eye + (A / s2[:, None, None]) @ A.transpose(1, 2))
    c = torch.linalg.solve_triangular(LB, (A @ (yt[None, :] / s2[:, None])[:, :, None]), upper=False)[:, :, 0]
    logdet = 0.5 * N * torch.log(s2) + torch.log(torch.diagonal(LB, dim1=1, dim2=2)).sum(1)
    quad = 0.5 * ((yt * yt).sum() / s2 - (c * c).sum(1))
    lp = -(0.5 * N * math.log(2.0 * math.pi) + logdet + quad + trace)
    for cval in (sf2, ls, s2):
        lp = lp + torch.log(cval) - cval                                   # Gamma(2, 1) at the constrained value
    lp = lp + torch.nn.functional.logsigmoid(xt).sum(1)                    # the transforms
    ok = (info1 == 0) & (info2 == 0) & torch.isfinite(lp)
    lp = torch.where(ok, lp, torch.full_like(lp, -math.inf))
    if not want_v:
        return lp.numpy()
    LBi = torch.linalg.solve_triangular(LB, eye.expand_as(LB), upper=False)
    m = (LBi.transpose(1, 2) @ c[:, :, None])[:, :, 0]                     # B^-1 u / s2 = LB^-T c
    return lp.numpy(), m.numpy(), (LBi * LBi).sum(1).numpy()               # diag(B^-1) = column norms of LB^-1


def logp_one(x, X, y, Z):
    """The same density at ONE point through the oracle's VFE bound (oracle.vfe_pymc3_order): the generator's independent check."""
    from oracle import vfe_oracle as O
    sp = lambda t: math.log1p(math.exp(-abs(t))) + max(t, 0.0)
    sf2, ls, s2 = sp(x[0]), sp(x[1]), NOISE_FLOOR + sp(x[2])
    F = float(O.vfe_pymc3_order(X, y, Z, [ls], math.sqrt(sf2), math.sqrt(s2), jitter=JITTER))
    return F + sum(math.log(c) - c for c in (sf2, ls, s2)) + sum(-sp(-t) for t in x)


def moments(X, y, Z, lo, hi, n, lp_max):
    # (the variance axis carries the Gamma prior's exp(-c) tail, ten times the width of the bulk: twice the nodes there)
    rules = [np.polynomial.legendre.leggauss(2 * n if k == 0 else n) for k in range(3)]
    nodes = [0.5 * (hi[k] - lo[k]) * rules[k][0] + 0.5 * (hi[k] + lo[k]) for k in range(3)]
    wts = [0.5 * (hi[k] - lo[k]) * rules[k][1] for k in range(3)]
    M = Z.shape[0]
    S0, S1, S2 = 0.0, np.zeros(3), np.zeros((3, 3))
    V1, V2 = np.zeros(M), np.zeros(M)
    rows = []
    for i in range(nodes[0].size):
        g1, g2 = np.meshgrid(nodes[1], nodes[2], indexing="ij")
        th = np.stack([np.full(g1.size, nodes[0][i]), g1.ravel(), g2.ravel()], 1)
        lp, m, bd = logp_batch(th, X, y, Z, want_v=True)
        p = np.exp(lp - lp_max) * (wts[0][i] * np.outer(wts[1], wts[2]).ravel())
        live = p > 0
        S0 += p.sum()
        S1 += p @ th
        S2 += th.T @ (th * p[:, None])
        V1 += p[live] @ m[live]
        V2 += p[live] @ (bd[live] + m[live] ** 2)
        rows.append((th, p))
    mean = S1 / S0
    cov = S2 / S0 - np.outer(mean, mean)
    m3, m4 = np.zeros(3), np.zeros(3)
    for th, p in rows:
        c = th - mean
        m3 += p @ c ** 3
        m4 += p @ c ** 4
    v_mean = V1 / S0
    return math.log(S0) + lp_max, mean, cov, m3 / S0, m4 / S0, v_mean, V2 / S0 - v_mean ** 2


def main():
    G = np.load(os.path.join(OUT, "rbf_d1_tiny.npz"))
    X, y, Z = G["X"], G["y"], G["Z"]
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform(-2.0, 4.0, 100), rng.uniform(0.0, 8.0, 100), rng.uniform(-6.0, 1.0, 100)], 1)
    ref = np.array([logp_one(p, X, y, Z) for p in pts])
    got = logp_batch(pts, X, y, Z)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() < 1e-8, err.max()
    ax = [np.linspace(-8.0, 64.0, 145), np.linspace(-4.0, 44.0, 97), np.linspace(-10.0, 4.0, 57)]   # (Gamma(2, 1) tails: exp(-c), not Gaussian)
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    lp = np.concatenate([logp_batch(g[i:i + 20000], X, y, Z) for i in range(0, g.shape[0], 20000)])
    lp_max = float(lp.max())
    keep = g[lp > lp_max - 38.0]
    lo, hi = keep.min(0) - 0.4, keep.max(0) + 0.4
    print("peak logp %.6f at %s ; box %s .. %s" % (lp_max, g[lp.argmax()], lo, hi))
    r = moments(X, y, Z, lo, hi, 112, lp_max)
    r2 = moments(X, y, Z, lo, hi, 72, lp_max)
    wid = 0.125 * (hi - lo)
    r3 = moments(X, y, Z, lo - wid, hi + wid, 112, lp_max)
    ev, mean, cov, m3, m4, v_mean, v_var = r
    print("log evidence %.12f ; mean %s ; sd %s" % (ev, mean, np.sqrt(np.diag(cov))))
    print("E[v] %s\nsd[v] %s" % (v_mean, np.sqrt(v_var)))
    for name, a in (("72 vs 112 nodes", r2), ("box + 25 %", r3)):
        dm, dc = float(np.max(np.abs(a[1] - mean))), float(np.max(np.abs(a[2] - cov)))
        dv, dvv = float(np.max(np.abs(a[5] - v_mean))), float(np.max(np.abs(a[6] - v_var)))
        print("  %-16s d(log Z) %.2e  d(mean) %.2e  d(cov) %.2e  d(E v) %.2e  d(Var v) %.2e" % (name, abs(a[0] - ev), dm, dc, dv, dvv))
        assert abs(a[0] - ev) < 1e-8 and dm < 1e-8 and dc < 1e-8 and dv < 1e-8 and dvv < 1e-8, name
    t, _ = np.polynomial.legendre.leggauss(24)
    face_max = -np.inf
    for k in range(3):
        others = [j for j in range(3) if j != k]
        a, b = np.meshgrid(*[0.5 * (hi[j] - lo[j]) * t + 0.5 * (hi[j] + lo[j]) for j in others], indexing="ij")
        for edge in (lo[k], hi[k]):
            th = np.zeros((a.size, 3))
            th[:, k] = edge
            th[:, others[0]] = a.ravel()
            th[:, others[1]] = b.ravel()
            face_max = max(face_max, float(logp_batch(th, X, y, Z).max()))
    print("  max logp on the faces: peak - %.1f" % (lp_max - face_max))
    assert lp_max - face_max > 30.0
    x_spot = np.round(mean, 1)
    np.savez(os.path.join(OUT, "posterior_sgpmc_d1_tiny.npz"), X=X, y=y, Z=Z, jitter=JITTER, box_lo=lo, box_hi=hi, log_evidence=ev,
             mean=mean, cov=cov, m3=m3, m4=m4, v_mean=v_mean, v_var=v_var, x_spot=x_spot, logp_spot=float(logp_batch(x_spot[None], X, y, Z)[0]),
             logp_peak=lp_max, nodes_per_axis=112)
    print("wrote posterior_sgpmc_d1_tiny.npz")


if __name__ == "__main__":
    main()
