"""Brute-force f64 numpy restatement of precision / recall / density / coverage (xmc_gan_amd/manifold.py, csrc/manifold.hip).

With d2(a, b) = |a - b|^2 (formed from the differences, in f64), real rows R [Nr, D], generated rows G [Ng, D] and k:

    rad2_X[i]  = the k-th smallest d2(X_i, X_j) over j != i  -- the row is excluded by INDEX, duplicates count as separate neighbours
    cnt_G[j]   = #{ i : d2(G_j, R_i) <= rad2_R[i] }      precision = mean(cnt_G > 0),   density = sum(cnt_G) / (k Ng)
    cnt_R[i]   = #{ j : d2(R_i, G_j) <= rad2_G[j] }      recall    = mean(cnt_R > 0)
    near2_R[i] = min_j d2(R_i, G_j)                       coverage  = mean(near2_R <= rad2_R)

Every comparison is <= on squared distances; no square root is taken.

Beside each count the reference returns `lo` and `hi`: the count with the comparison tightened / loosened by the band
TAU * (|a|^2 + |b|^2), and the same for the coverage decision.  A row is AMBIGUOUS when lo != hi: an f32 kernel may land on either side.
TAU = 2e-6 is twice the bound of the kernel's error: the f32 MFMA chain errs by at most 3.5e-7 * sum|a_d b_d| up to 4096 terms, sum|a_d b_d|
<= (|a|^2 + |b|^2) / 2 and the dot enters d2 twice, so 3.5e-7 * (|a|^2 + |b|^2); the two norms and the radius add about 1e-7 * (|a|^2 +
|b|^2) each: under 1e-6 * (|a|^2 + |b|^2) in all.
"""
import numpy as np

TAU = 2e-6


def sqdist(a, b):
    """d2 [Na, Nb] in f64.  Narrow rows: from the differences.  Wide rows (D > 64, where the [Na, Nb, D] differences would take seconds and
    gigabytes): |a|^2 + |b|^2 - 2 a.b in f64, whose cancellation error is 1e-16 * (|a|^2 + |b|^2) -- ten orders below the band TAU"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape[1] > 64:
        return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)
    d = a[:, None, :] - b[None, :, :]
    return np.einsum("ijk,ijk->ij", d, d)


def knn_radius2(x, k):
    """rad2 [N]: the k-th smallest d2 to the other rows"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    assert 1 <= k and n >= k + 1
    d = sqdist(x, x)
    d[np.arange(n), np.arange(n)] = np.inf           # by index: a duplicate row elsewhere stays, at distance 0
    return np.sort(d, axis=1)[:, k - 1]


def count(a, b, rb2, tau=TAU):
    """dict(count, lo, hi [Na] ints; near2 [Na]; band [Na, Nb]) of the query rows a against the rows b with radii rb2"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = sqdist(a, b)
    band = tau * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
    rb2 = np.asarray(rb2, np.float64)[None, :]
    return dict(count=(d <= rb2).sum(1), lo=(d <= rb2 - band).sum(1), hi=(d <= rb2 + band).sum(1), near2=d.min(1), d2=d, band=band)


def reference(real, fake, k, tau=TAU):
    """everything of the definitions above, with the band versions of every decision"""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    rad_r, rad_g = knn_radius2(real, k), knn_radius2(fake, k)
    g = count(fake, real, rad_r, tau)                # generated rows inside real balls
    r = count(real, fake, rad_g, tau)                # real rows inside generated balls
    # coverage: near2_R[i] <= rad2_R[i]; the band of row i is the one of its nearest generated row (and of every row that close)
    slack = (r["d2"] - rad_r[:, None])
    cov = r["near2"] <= rad_r
    cov_lo = (slack <= -r["band"]).any(1)
    cov_hi = (slack <= r["band"]).any(1)
    ng, nr = fake.shape[0], real.shape[0]
    out = dict(rad2_r=rad_r, rad2_g=rad_g, cnt_g=g["count"], cnt_g_lo=g["lo"], cnt_g_hi=g["hi"], cnt_r=r["count"], cnt_r_lo=r["lo"],
               cnt_r_hi=r["hi"], near2_r=r["near2"], near2_g=g["near2"], cov=cov, cov_lo=cov_lo, cov_hi=cov_hi,
               precision=float((g["count"] > 0).mean()), recall=float((r["count"] > 0).mean()),
               density=float(g["count"].sum()) / (k * ng), coverage=float(cov.mean()), k=k, n_real=nr, n_fake=ng)
    out["ambiguous_g"] = g["lo"] != g["hi"]
    out["ambiguous_r"] = (r["lo"] != r["hi"]) | (cov_lo != cov_hi)
    return out


def lattice(nr=130, ng=67, d=12, seed=9):
    """integer rows 0..3: every product and sum of the GEMM form is exact in f32, and many radii are tied"""
    g = np.random.default_rng(seed)
    return g.integers(0, 4, (nr, d)).astype(np.float32), g.integers(0, 4, (ng, d)).astype(np.float32)


def gaussian(nr, ng, d, seed):
    g = np.random.default_rng(seed)
    real = g.standard_normal((nr, d)).astype(np.float32)
    fake = (0.9 * g.standard_normal((ng, d)) + 0.3).astype(np.float32)
    return real, fake


def lowrank(nr, ng, d, seed, rank=16, noise=0.02):
    """non-negative rows near a rank-16 cone: what pooled ReLU features look like (isotropic Gaussians at D = 2048 concentrate: every
    decision becomes marginal)"""
    g = np.random.default_rng(seed)
    basis = g.standard_normal((rank, d))

    def rows(n, shift):
        w = g.standard_normal((n, rank)) + shift
        return np.maximum(w @ basis / np.sqrt(rank) + noise * g.standard_normal((n, d)), 0.0).astype(np.float32)
    return rows(nr, 0.0), rows(ng, 0.15)
