"""Host side of the differentiable augmentation of the discriminator's inputs (Zhao et al., "Differentiable Augmentation for
Data-Efficient GAN Training"): the per-image parameter rows that ``ops.diffaug`` (csrc/augment.hip) reads.

One object per training run owns ONE static device tensor ``params`` f32 [3*batch, 8], row = (b, s, c, tx, ty, cy, cx, 0):

    rows [0, B)     the real images of the discriminator step (the MA-GP pass reuses them)
    rows [B, 2B)    the generated images of the discriminator step
    rows [2B, 3B)   the generator step (its generated images and, under ENCODER_LOSS.DISC, its second pass over the real ones)

`refresh()` draws every row on the host and copies them in with one asynchronous copy.  The loop calls it before each iteration,
OUTSIDE any graph capture; the kernels read the rows inside the graph, so a replay sees the new draw.
"""
import torch

COMPONENTS = ("color", "translation", "cutout")
COLS = 8                    # (b, s, c, tx, ty, cy, cx, 0)


def parse_policy(policy):
    """'color,translation,cutout' (any subset, any order) -> tuple of names; unknown names raise ValueError, '' is the empty policy"""
    names = tuple(t.strip() for t in str(policy or "").split(",") if t.strip())
    for t in names:
        if t not in COMPONENTS:
            raise ValueError(f"unknown DiffAugment component {t!r}: choose from {', '.join(COMPONENTS)}")
    return tuple(t for t in COMPONENTS if t in names)


class DiffAugment:
    def __init__(self, policy, batch, height, width, device, seed, rank=0):
        self.policy = parse_policy(policy)
        if not self.policy:
            raise ValueError("empty DiffAugment policy: pass None instead of a DiffAugment object to switch the augmentation off")
        self.batch, self.height, self.width = int(batch), int(height), int(width)
        self.device = torch.device(device)
        self.color = "color" in self.policy               # ops.diffaug(color=): without it the sums launch is skipped
        # the cutout square's side: half of the image (of its smaller side, so that the square fits a non-square map)
        self.cut = int(min(self.height, self.width) * 0.5 + 0.5) if "cutout" in self.policy else 0
        # a CPU generator, as the noise is drawn (train_gan.py:197); one stream per (seed, rank, ...) so that ranks augment differently
        self.gen = torch.Generator()
        self.seed(seed, rank)
        self.params = torch.zeros((3 * self.batch, COLS), dtype=torch.float32, device=self.device)
        self.params.copy_(self.identity_rows(3 * self.batch))

    def seed(self, *key):
        """(seed, rank) at construction; (seed, rank, epoch) on a resume: the draws restart from the epoch, they are not continued"""
        s = 0
        for k in key:
            s = (s * 1000003 + int(k) + 0x9E3779B9) % (2 ** 63 - 1)
        self.gen.manual_seed(s)

    @staticmethod
    def identity_rows(n):
        rows = torch.zeros((n, COLS), dtype=torch.float32)
        rows[:, 1] = 1.0
        rows[:, 2] = 1.0
        return rows

    def sample(self, n=None):
        """n (default 3*batch) rows on the host.  A component outside the policy keeps its identity value: b = 0, s = 1, c = 1; tx = ty = 0;
        cut = 0 (then cy, cx are not read and stay 0)."""
        n = 3 * self.batch if n is None else int(n)
        g, H, W = self.gen, self.height, self.width
        rows = self.identity_rows(n)
        if "color" in self.policy:
            rows[:, 0] = torch.rand(n, generator=g) - 0.5
            rows[:, 1] = torch.rand(n, generator=g) * 2.0
            rows[:, 2] = torch.rand(n, generator=g) + 0.5
        if "translation" in self.policy:
            rw, rh = int(W * 0.125 + 0.5), int(H * 0.125 + 0.5)
            rows[:, 3] = torch.randint(-rw, rw + 1, (n,), generator=g).float()
            rows[:, 4] = torch.randint(-rh, rh + 1, (n,), generator=g).float()
        if "cutout" in self.policy:
            cut = self.cut
            rows[:, 5] = (torch.randint(0, H + (1 - cut % 2), (n,), generator=g) - cut // 2).float()
            rows[:, 6] = (torch.randint(0, W + (1 - cut % 2), (n,), generator=g) - cut // 2).float()
        return rows

    def refresh(self):
        """new rows for the next iteration: drawn on the host, one non-blocking copy from pinned memory into the static device tensor"""
        rows = self.sample()
        if self.device.type == "cuda":
            host = torch.empty(rows.shape, dtype=torch.float32, pin_memory=True)     # (the caching host allocator keeps the block until the copy is done)
            host.copy_(rows)
            rows = host
        self.params.copy_(rows, non_blocking=True)

    def set_identity(self):
        """every row the identity (tests: the augmented iteration must then reproduce the plain one)"""
        self.params.copy_(self.identity_rows(3 * self.batch))

    # the three row blocks
    def rows_d(self):
        return self.params[:2 * self.batch]

    def rows_real(self):
        return self.params[:self.batch]

    def rows_fake(self):
        return self.params[self.batch:2 * self.batch]

    def rows_g(self):
        return self.params[2 * self.batch:]

    def __call__(self, x_nhwc8, rows):
        from . import ops
        return ops.diffaug(x_nhwc8, rows, self.cut, color=self.color)
