"""Plain-torch restatement of AttnGAN's DAMSM image encoder (CNN_ENCODER), for the tests (a helper, not a test): torchvision's Inception-v3
up to Mixed_7c -- tests/fid_ref.py's layer table with the two places where torchvision differs from the FID network, every ``branch_pool``
averaging with count_include_pad=True and Mixed_7c's pool branch being that average too -- then ``emb_features`` (1x1 convolution without
bias) on Mixed_6e's output and ``emb_cnn_code`` (linear) on the pooled Mixed_7c output.  CPU, f64, NCHW.  `random_state_dict(seed, nef)`
makes weights in AttnGAN's key layout.  Shares no code with xmc_gan_amd/ or xmc_gan/model/encoder.py."""
import torch
import torch.nn.functional as F

import fid_ref

# gains of the two random projections over a variance-preserving 1 / sqrt(fan_in): their inputs are post-ReLU (all positive, a mean of
# about 0.5 that zero-mean rows cancel), and these make the codes and the projected features of order 1
CODE_GAIN, FEATURE_GAIN = 4.0, 4.0


def random_state_dict(seed, nef=32):
    """f32 state dict with CNN_ENCODER's keys: the 94 BasicConv2d layers of `fid_ref.random_state_dict` (no ``fc``), ``emb_features.weight``
    [nef,768,1,1] ~ N(0, FEATURE_GAIN^2 / 768), ``emb_cnn_code.weight`` [nef,2048] ~ N(0, CODE_GAIN^2 / 2048) and its bias ~ N(0, 0.1)"""
    sd = {k: v for k, v in fid_ref.random_state_dict(seed).items() if not k.startswith("fc.")}
    g = torch.Generator().manual_seed(seed + 1000)
    sd["emb_features.weight"] = torch.randn(nef, 768, 1, 1, generator=g) * (FEATURE_GAIN / 768 ** 0.5)
    sd["emb_cnn_code.weight"] = torch.randn(nef, 2048, generator=g) * (CODE_GAIN / 2048 ** 0.5)
    sd["emb_cnn_code.bias"] = 0.1 * torch.randn(nef, generator=g)
    return sd


def structured_images(n, side, seed):
    """uint8 [n,side,side,3]: per image a random hard-edged 4x4 colour pattern at a random contrast over tinted noise -- images whose codes
    differ visibly (about a tenth of their size; uniform noise images all have the same statistics and so nearly the same code, and a
    random network carries smooth differences no further)"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(n, 3, 4, 4, generator=g)
    blocks = (F.interpolate(coarse, size=(side, side), mode="bilinear", align_corners=False) > 0.5).float()
    noise = torch.rand(n, 3, side, side, generator=g)
    contrast, tint = torch.rand(n, 1, 1, 1, generator=g), torch.rand(n, 3, 1, 1, generator=g)
    x = 255.0 * (blocks * contrast + tint * (1.0 - contrast) * noise)
    return x.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class Reference(fid_ref.Reference):
    """the encoder on the CPU in f64"""

    @staticmethod
    def avg(x):
        return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=True)

    def block(self, m, x):
        if m != "Mixed_7c":
            return super().block(m, x)            # (5b .. 7b take `avg` above; 6a and 7a have no average)
        b3 = self.conv(m + ".branch3x3_1", x)
        b3 = torch.cat([self.conv(m + ".branch3x3_2a", b3), self.conv(m + ".branch3x3_2b", b3)], 1)
        bd = self.seq(m, ["branch3x3dbl_1", "branch3x3dbl_2"], x)
        bd = torch.cat([self.conv(m + ".branch3x3dbl_3a", bd), self.conv(m + ".branch3x3dbl_3b", bd)], 1)
        return torch.cat([self.conv(m + ".branch1x1", x), b3, bd, self.conv(m + ".branch_pool", self.avg(x))], 1)

    def forward(self, x, resize_to=299):
        """f64 [B,3,H,W] in [-1, 1] -> (features [B,nef,h,w], cnn_code [B,nef]); upstream resizes to 299 (h = w = 17)"""
        with torch.no_grad():
            x = x.double()
            if resize_to is not None:
                x = F.interpolate(x, size=(resize_to, resize_to), mode="bilinear", align_corners=False)
            for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
                x = self.conv(n, x)
            x = F.max_pool2d(x, 3, stride=2)
            x = self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", x))
            x = F.max_pool2d(x, 3, stride=2)
            for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = self.block(m, x)
            features = x
            for m in ("Mixed_7a", "Mixed_7b", "Mixed_7c"):
                x = self.block(m, x)
            pooled = F.avg_pool2d(x, kernel_size=8).flatten(1) if tuple(x.shape[2:]) == (8, 8) else x.mean((2, 3))
            code = F.linear(pooled, self.sd["emb_cnn_code.weight"], self.sd["emb_cnn_code.bias"])
            return F.conv2d(features, self.sd["emb_features.weight"]), code

    def forward_u8(self, u8_nhwc, resize_to=299):
        """uint8 [N,H,W,3] -> the same pair, from 2 * (b / 255) - 1 (resized after the scaling, as CNN_ENCODER.forward sees it; the resize
        is linear with weights that sum to 1, so the order does not matter beyond rounding)"""
        return self.forward(2.0 * (torch.as_tensor(u8_nhwc).permute(0, 3, 1, 2).double() / 255.0) - 1.0, resize_to)


def cosine_scores(img, txt, cand, eps=1e-8):
    """f64 restatement of the retrieval: score[n][k] = <img n, txt c> / max(|img n| |txt c|, eps), c = cand[n][k]; rank[n] = the number of
    k >= 1 with score[n][k] > score[n][0] (K when score[n][0] is NaN)"""
    img, txt, cand = img.double(), txt.double(), torch.as_tensor(cand).long()
    rows = txt[cand]                                                        # [N,K,D]
    dot = (img[:, None, :] * rows).sum(-1)
    score = dot / (img.norm(dim=1)[:, None] * rows.norm(dim=2)).clamp(min=eps)
    rank = (score[:, 1:] > score[:, :1]).sum(1)
    rank = torch.where(torch.isnan(score[:, 0]), torch.full_like(rank, cand.shape[1]), rank)
    return score, rank
