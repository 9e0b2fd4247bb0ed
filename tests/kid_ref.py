"""Plain numpy f64 restatement of the Kernel Inception Distance and the Inception Score (xmc_gan_amd/manifold.py `kid`, xmc_gan_amd/fid.py
`InceptionScore`, csrc/kid.hip), written from the definitions:

KID (Binkowski et al. 2018, torch-fidelity's defaults).  k(x, y) = (x.y / D + 1)^3.  For S subsets of m rows per side, subset s being the
bank rows idx_real[s] / idx_fake[s]:

    XX_s = sum over ordered pairs i != j of k(X_i, X_j)        (i, j are POSITIONS in the subset: two positions that name the same bank
    YY_s = the same over the generated subset                   row are a pair, and it counts)
    XY_s = sum over all m^2 pairs of k(X_i, Y_j)
    MMD2_s = (XX_s + YY_s) / (m (m - 1)) - 2 XY_s / m^2         KID = mean_s MMD2_s, spread = np.std (ddof 0)

The draw: m = min(size, n_real, n_fake); one generator np.random.default_rng([seed, 0x4B4944]); per subset the real indices first, then
the generated ones, each by rng.choice(n, m, replace=False).

IS (Salimans et al. 2016).  p(y|x) = softmax of a row of logits, in f64.  The N rows are cut into `splits` consecutive parts, part s = rows
[s N // splits, (s + 1) N // splits); a part scores exp(mean_x sum_y p(y|x) (log p(y|x) - log p_s(y))) with p_s the part's mean of p(y|x);
IS = the mean over the parts, spread = np.std (ddof 0).  No shuffling.
"""
import numpy as np

KID_STREAM = 0x4B4944


def kernel(x, y):
    """k [Nx, Ny] in f64; the cube as two products"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    t = x @ y.T / x.shape[1] + 1.0
    return t * t * t


def subsets(n_real, n_fake, count=100, size=1000, seed=0):
    m = min(size, n_real, n_fake)
    if m < 2:
        raise ValueError("fewer than two rows")
    rng = np.random.default_rng([seed, KID_STREAM])
    idx_r, idx_f = [], []
    for _ in range(count):
        idx_r.append(rng.choice(n_real, m, replace=False))
        idx_f.append(rng.choice(n_fake, m, replace=False))
    return np.asarray(idx_r, np.int32), np.asarray(idx_f, np.int32)


def poly_mmd_sums(real, fake, idx_real, idx_fake):
    """[S, 3] f64: XX_s, YY_s, XY_s"""
    idx_real, idx_fake = np.asarray(idx_real), np.asarray(idx_fake)
    out = np.zeros((idx_real.shape[0], 3), np.float64)
    for s in range(idx_real.shape[0]):
        x, y = np.asarray(real, np.float64)[idx_real[s]], np.asarray(fake, np.float64)[idx_fake[s]]
        kxx, kyy, kxy = kernel(x, x), kernel(y, y), kernel(x, y)
        out[s] = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()
    return out


def poly_mmd_sums_loop(real, fake, idx_real, idx_fake):
    """the same by a double loop over positions, one pair at a time (tiny inputs: the check of `poly_mmd_sums`)"""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    d = real.shape[1]
    out = np.zeros((len(idx_real), 3), np.float64)
    for s in range(len(idx_real)):
        m = len(idx_real[s])
        for i in range(m):
            for j in range(m):
                xi, xj, yi, yj = real[idx_real[s][i]], real[idx_real[s][j]], fake[idx_fake[s][i]], fake[idx_fake[s][j]]
                if i != j:
                    out[s, 0] += (float(xi @ xj) / d + 1.0) ** 3
                    out[s, 1] += (float(yi @ yj) / d + 1.0) ** 3
                out[s, 2] += (float(xi @ yj) / d + 1.0) ** 3
    return out


def mmd2(sums, m):
    sums = np.asarray(sums, np.float64)
    return (sums[:, 0] + sums[:, 1]) / (m * (m - 1.0)) - 2.0 * sums[:, 2] / (float(m) * m)


def kid(real, fake, idx_real, idx_fake):
    """(KID, spread) over the given subsets"""
    v = mmd2(poly_mmd_sums(real, fake, idx_real, idx_fake), np.asarray(idx_real).shape[1])
    return float(v.mean()), float(v.std())


def assert_exact_in_f32(real, fake):
    """the precondition of the bit-for-bit cases, from the data alone: every kernel value among these rows survives a round trip through
    float32 (then so do the dot product, t = dot / D + 1 and t^2, which have fewer digits; and f64 adds them without rounding)"""
    x = np.concatenate([np.asarray(real, np.float64), np.asarray(fake, np.float64)])
    k = kernel(x, x)
    assert np.array_equal(k.astype(np.float32).astype(np.float64), k), "a kernel value of this lattice is not a float32"
    t = x @ x.T / x.shape[1] + 1.0
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and k.sum() < 2.0 ** 52 / (x.shape[1] ** 3)


def split_bounds(n, splits):
    if splits < 1 or n < splits:
        raise ValueError("fewer rows than splits")
    return [(s * n // splits, (s + 1) * n // splits) for s in range(splits)]


def inception_score(logits, splits=10):
    """(IS, spread, the per-part scores)"""
    z = np.asarray(logits, np.float64)
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    scores = []
    for lo, hi in split_bounds(z.shape[0], splits):
        ps = p[lo:hi].mean(axis=0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.where(p[lo:hi] > 0, p[lo:hi] * (logp[lo:hi] - np.log(ps)), 0.0)
        scores.append(np.exp(terms.sum(axis=1).mean()))
    scores = np.asarray(scores, np.float64)
    return float(scores.mean()), float(scores.std()), scores


def inception_score_loop(logits, splits):
    """the per-part scores by loops over rows and classes (tiny inputs: the check of `inception_score`)"""
    import math
    z = np.asarray(logits, np.float64)
    out = []
    for lo, hi in split_bounds(z.shape[0], splits):
        probs = []
        for x in z[lo:hi]:
            mx = max(x)
            e = [math.exp(v - mx) for v in x]
            probs.append([v / sum(e) for v in e])
        c = z.shape[1]
        marg = [sum(p[y] for p in probs) / len(probs) for y in range(c)]
        kl = [sum(p[y] * (math.log(p[y]) - math.log(marg[y])) for y in range(c) if p[y] > 0) for p in probs]
        out.append(math.exp(sum(kl) / len(kl)))
    return np.asarray(out)
