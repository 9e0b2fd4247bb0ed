"""Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of a generated set against a real
one: k-nearest-neighbour statistics of feature rows, on the kernels of csrc/manifold.hip.

The rows are the 2048-d pool3 features `xmc_gan_amd.fid.InceptionFID` returns, so one Inception pass serves FID and these four numbers.
(They are NOT the VGG-16 features of the published precision / recall figures: values are comparable among runs of this project only.)

With d2(a, b) = |a - b|^2, R [Nr, D] real rows, G [Ng, D] generated rows:

    rad2_X[i]  = the k-th smallest d2(X_i, X_j) over j != i (excluded by index; duplicates are neighbours at distance 0)
    cnt_G[j]   = #{ i : d2(G_j, R_i) <= rad2_R[i] }      precision = mean(cnt_G > 0),   density = sum(cnt_G) / (k Ng)
    cnt_R[i]   = #{ j : d2(R_i, G_j) <= rad2_G[j] }      recall    = mean(cnt_R > 0)
    near2_R[i] = min_j d2(R_i, G_j)                       coverage  = mean(near2_R <= rad2_R)

``FeatureBank`` keeps rows on the device; ``prdc`` runs two radius and two count launches (the N x N matrix exists nowhere) and reduces the
per-row results on the host in f64; ``prdc_from_counts`` is that host reduction alone.

``kid`` is the Kernel Inception Distance (Binkowski et al. 2018) of the same rows, on csrc/kid.hip: the polynomial kernel
k(x, y) = (x.y / D + 1)^3 and, over ``subsets`` subsets of m = min(subset_size, Nr, Ng) rows per side drawn without replacement
(``kid_subsets``), the unbiased

    MMD^2 = (sum_{i != j} k(X_i, X_j) + sum_{i != j} k(Y_i, Y_j)) / (m (m - 1)) - 2 sum_{i, j} k(X_i, Y_j) / m^2

whose mean and standard deviation (ddof 0) over the subsets are reported.  The kernel, the subset count and size are torch-fidelity's
defaults; the draw is this project's own, so a value differs from torch-fidelity's by sampling noise only -- the noise ``std`` shows.
"""
import os

import numpy as np
import torch

from . import ops

DIMS = 2048
MAX_K = 16


class FeatureBank:
    """feature rows [n, dims] f32 on the device, appended batch by batch; the storage grows by doubling"""

    def __init__(self, dims=DIMS, device="cuda"):
        self.dims, self.device, self.n = int(dims), torch.device(device), 0
        self._buf = None

    def update(self, features):
        f = torch.as_tensor(features)
        if f.dim() != 2 or f.shape[1] != self.dims or f.dtype != torch.float32:
            raise ValueError(f"FeatureBank: f32 rows [B,{self.dims}] expected, got {f.dtype} {tuple(f.shape)}")
        need = self.n + f.shape[0]
        if self._buf is None or need > self._buf.shape[0]:
            cap = max(need, 2 * (0 if self._buf is None else self._buf.shape[0]), 256)
            buf = torch.empty((cap, self.dims), dtype=torch.float32, device=self.device)
            if self.n:
                buf[:self.n] = self._buf[:self.n]
            self._buf = buf
        self._buf[self.n:need] = f.detach().to(self.device)
        self.n = need

    def rows(self):
        """the rows held so far, [n, dims] (a view of the storage)"""
        if self._buf is None:
            return torch.empty((0, self.dims), dtype=torch.float32, device=self.device)
        return self._buf[:self.n]

    def save(self, path):
        save_features(path, self.rows().cpu().numpy())

    @classmethod
    def load(cls, path, device="cuda"):
        feats = load_features(path)
        bank = cls(feats.shape[1], device)
        if feats.shape[0]:
            bank.update(torch.from_numpy(feats))
        return bank


def save_features(path, features):
    """an .npz with ``features`` [N,D] f32 and ``n``"""
    features = np.ascontiguousarray(features, np.float32)
    with open(path, "wb") as f:           # (a file object: np.savez appends nothing to the name)
        np.savez(f, features=features, n=np.int64(features.shape[0]))


def load_features(path):
    """the [N,D] f32 rows of a file written by `save_features`; a statistics file (``mu``, ``sigma``) is refused: moments hold no rows"""
    with np.load(path) as z:
        if "features" not in z.files:
            if "mu" in z.files and "sigma" in z.files:
                raise ValueError(f"{path} is a statistics file (mu, sigma: what pytorch_fid and FID cache): it holds only moments, and precision / "
                                 "recall / density / coverage need the feature rows themselves; write them with --save_features")
            raise ValueError(f"{path}: a feature file holds 'features', this one holds {z.files}")
        feats = np.ascontiguousarray(z["features"], np.float32)
        n = int(z["n"]) if "n" in z.files else None
    if feats.ndim != 2 or (n is not None and n != feats.shape[0]):
        raise ValueError(f"{path}: features {feats.shape} with n = {n} are not [n, D] rows")
    return feats


def prdc_from_counts(cnt_g, cnt_r, near2_r, rad2_r, k):
    """the four numbers from the per-row results (arrays on the host), in f64:
    cnt_g [Ng] ints, cnt_r [Nr] ints, near2_r [Nr] and rad2_r [Nr] squared distances"""
    cnt_g, cnt_r = np.asarray(cnt_g, np.int64), np.asarray(cnt_r, np.int64)
    near2_r, rad2_r = np.asarray(near2_r), np.asarray(rad2_r)
    k = int(k)
    if cnt_g.ndim != 1 or cnt_r.ndim != 1 or near2_r.shape != cnt_r.shape or rad2_r.shape != cnt_r.shape or not cnt_g.size or not cnt_r.size:
        raise ValueError(f"prdc_from_counts: shapes {cnt_g.shape} {cnt_r.shape} {near2_r.shape} {rad2_r.shape}")
    if k < 1:
        raise ValueError(f"prdc_from_counts: k = {k}")
    ng, nr = cnt_g.size, cnt_r.size
    return dict(precision=float(np.count_nonzero(cnt_g > 0)) / ng, recall=float(np.count_nonzero(cnt_r > 0)) / nr,
                density=float(cnt_g.sum()) / (float(k) * ng), coverage=float(np.count_nonzero(near2_r <= rad2_r)) / nr,
                k=k, n_real=int(nr), n_fake=int(ng))


def _rows(x):
    return x.rows() if isinstance(x, FeatureBank) else x


def prdc(real, fake, k=5):
    """precision, recall, density and coverage of ``fake`` against ``real`` (f32 [N,D] device tensors or `FeatureBank`s; D % 4 == 0,
    D <= 4096; both sets need at least k + 1 rows, k <= 16) -> dict(precision, recall, density, coverage, k, n_real, n_fake)"""
    real, fake, k = _rows(real), _rows(fake), int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"prdc: k = {k}; 1 <= k <= {MAX_K} expected")
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1]:
        raise ValueError(f"prdc: feature rows [Nr,D] and [Ng,D] expected, got {tuple(real.shape)} and {tuple(fake.shape)}")
    if min(real.shape[0], fake.shape[0]) < k + 1:
        raise ValueError(f"prdc: k = {k} needs at least {k + 1} rows in both sets, got {real.shape[0]} real and {fake.shape[0]} generated")
    rad2_r, rad2_g = ops.knn_radius2(real, k), ops.knn_radius2(fake, k)
    cnt_g, _ = ops.manifold_count(fake, real, rad2_r)
    cnt_r, near2_r = ops.manifold_count(real, fake, rad2_g)
    return prdc_from_counts(cnt_g.cpu().numpy(), cnt_r.cpu().numpy(), near2_r.cpu().numpy(), rad2_r.cpu().numpy(), k)


KID_SUBSETS, KID_SUBSET_SIZE = 100, 1000


def kid_subsets(n_real, n_fake, subsets=KID_SUBSETS, size=KID_SUBSET_SIZE, seed=0):
    """the subsets of KID: two int32 [subsets, m] tables of rows, m = min(size, n_real, n_fake), every row of a table drawn without
    replacement.  One generator, ``np.random.default_rng([seed, 0x4B4944])``; per subset the real indices first, then the generated ones.
    ValueError: m < 2 or subsets < 1."""
    n_real, n_fake, subsets, size = int(n_real), int(n_fake), int(subsets), int(size)
    m = min(size, n_real, n_fake)
    if m < 2:
        raise ValueError(f"KID needs at least two rows per side and subset, got {n_real} real and {n_fake} generated rows at subset size {size}")
    if subsets < 1:
        raise ValueError(f"KID: {subsets} subsets")
    rng = np.random.default_rng([int(seed), 0x4B4944])
    idx_r, idx_f = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(subsets):
        idx_r[s] = rng.choice(n_real, m, replace=False)
        idx_f[s] = rng.choice(n_fake, m, replace=False)
    return idx_r, idx_f


def kid_from_sums(sums, m):
    """(mean, std with ddof 0) over the subsets of the unbiased MMD^2 from the [S,3] sums of `ops.poly_mmd_sums`, in f64 on the host"""
    sums, m = np.asarray(sums, np.float64), int(m)
    mmd2 = (sums[:, 0] + sums[:, 1]) / (m * (m - 1.0)) - 2.0 * sums[:, 2] / (float(m) * m)
    return float(mmd2.mean()), float(mmd2.std())


def kid(real, fake, subsets=KID_SUBSETS, subset_size=KID_SUBSET_SIZE, seed=0):
    """Kernel Inception Distance of ``fake`` against ``real`` (f32 [N,D] device tensors or `FeatureBank`s; D % 4 == 0, 4 <= D <= 4096)
    -> dict(kid, std, subsets, subset_size, n_real, n_fake); ``subset_size`` is the m that was used.  ValueError: fewer than two rows."""
    real, fake = _rows(real), _rows(fake)
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1]:
        raise ValueError(f"kid: feature rows [Nr,D] and [Ng,D] expected, got {tuple(real.shape)} and {tuple(fake.shape)}")
    idx_r, idx_f = kid_subsets(real.shape[0], fake.shape[0], subsets, subset_size, seed)
    m = idx_r.shape[1]
    sums = ops.poly_mmd_sums(real, fake, torch.from_numpy(idx_r), torch.from_numpy(idx_f))
    mean, std = kid_from_sums(sums.cpu().numpy(), m)
    return dict(kid=mean, std=std, subsets=int(idx_r.shape[0]), subset_size=int(m), n_real=int(real.shape[0]), n_fake=int(fake.shape[0]))


def bank_of_dir(directory, extractor, batch=100):
    """`FeatureBank` of the image files of ``directory`` in sorted order (`xmc_gan_amd.fid.features_of_dir`)"""
    from .fid import accumulate, features_of_dir
    return accumulate(FeatureBank(DIMS, extractor.device), features_of_dir(directory, extractor, batch))


def bank_of(path, extractor, batch=100, device="cuda"):
    """`FeatureBank` of an image directory or of an .npz feature file"""
    if os.path.isdir(path):
        return bank_of_dir(path, extractor, batch)
    return FeatureBank.load(path, device)
