"""xmc_gan_amd.ops, layer 3: the forward-only operators outside autograd.  Plain functions that check their arguments and launch: images as
uint8, the image pool and the caption gather of the data feed, the metric kernels (FID, R-precision, the manifold metrics, KID, IS) and the
frozen encoders' front ends (the RNN text encoder, the RoBERTa and CLIP wrappers, Pillow's resize tables).  Imports `_config`."""
import math
import numpy as np
import torch
from .. import lib as L
from ._config import _code, _need_cuda, _p, _st, act_dtype


# ------------------------------------------------------------------------------------------ images as uint8 pixels (csrc/image.hip)
def _image_arg(x8, what):
    """the engine-layout image of the two wrappers below, checked: they are plain functions outside autograd"""
    _need_cuda(x8)
    if x8.dim() != 4 or x8.shape[-1] != 8:
        raise ValueError(f"{what}: an engine-layout image [N,H,W,8] expected, got {tuple(x8.shape)}")
    if x8.requires_grad:
        raise ValueError(f"{what} is not differentiable: detach the image first")
    if x8.dtype != act_dtype():
        raise TypeError(f"{what}: {x8.dtype} image in the {act_dtype()} mode (ops.set_precision)")
    return x8.contiguous()


def _u8_out(out, shape, device, what):
    """the uint8 destination: a new tensor, or the caller's (any byte address: the kernels ask for no alignment of it)"""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: out must be a contiguous uint8 {tuple(shape)} tensor on {device}")
    return out


def image_to_u8(x8, out=None):
    """[N,H,W,8] -> uint8 [N,H,W,3] = trunc((x + 1) * 127.5): the bytes of `utils.visual.to_uint8_hwc`, made on the device"""
    x8 = _image_arg(x8, "image_to_u8")
    N, H, W, _ = x8.shape
    y = _u8_out(out, (N, H, W, 3), x8.device, "image_to_u8")
    L.call("xmc_image_to_u8", _p(x8), _p(y), N, H, W, _code(x8.dtype), _st())
    return y


def image_grid_u8(x8, nrow=8, padding=2, out=None):
    """[N,H,W,8] -> uint8 [Hg,Wg,3]: the bytes `utils.visual.save_image(x, normalize=True, scale_each=True)` encodes (every image min-max
    scaled on its own, `nrow` per row, `padding` black pixels around each; one image: the image alone).  Two launches: the per-image
    partial (min, max), then the grid, which writes every byte of it.  ``out``: a contiguous uint8 destination of the grid's size."""
    x8 = _image_arg(x8, "image_grid_u8")
    N, H, W, _ = x8.shape
    nrow, padding = int(nrow), int(padding)
    if nrow < 1 or padding < 0:
        raise ValueError(f"image_grid_u8: nrow {nrow}, padding {padding}")
    pad = 0 if N == 1 else padding
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    shape = ((H + pad) * ymaps + pad, (W + pad) * xmaps + pad, 3)
    out = _u8_out(out, shape, x8.device, "image_grid_u8")
    parts = torch.empty((N, L.DIFFAUG_PARTS, 2), dtype=torch.float32, device=x8.device)
    L.call("xmc_image_minmax", _p(x8), _p(parts), N, H, W, _code(x8.dtype), _st())
    L.call("xmc_image_grid_u8", _p(x8), _p(parts), _p(out), N, H, W, nrow, padding, _code(x8.dtype), _st())
    return out


# ------------------------------------------------------------------------------------------ training batches from a uint8 image pool (csrc/datafeed.hip)
class HostMirror:
    """A small integer array that lives twice: ``host`` (numpy, drawn or loaded there) and ``dev`` (its device copy, what a kernel reads).
    `crop_flip_normalize` checks the host copy before it launches on the device copy, without a read-back."""

    def __init__(self, host, device=None, dev=None):
        """``device``: upload ``host`` there; or ``dev``: the device copy that already exists (a slice of a larger upload)"""
        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host).to(device) if dev is None else dev


def validate_crop_params(params, hw, size):
    """The bounds `crop_flip_normalize` needs, checked on host arrays: params int32 [B,4] = (image index, top, left, flip) against
    hw int32 [N,2] = (height, width): 0 <= index < N, 0 <= top <= h - size, 0 <= left <= w - size, flip in {0, 1}.  ValueError names the
    first offending row."""
    params, hw = np.asarray(params), np.asarray(hw)
    if params.ndim != 2 or params.shape[1] != 4 or params.shape[0] < 1 or params.dtype != np.int32:
        raise ValueError(f"crop params: int32 [B,4] with B >= 1 expected, got {params.dtype} {params.shape}")
    if hw.ndim != 2 or hw.shape[1] != 2 or hw.shape[0] < 1 or hw.dtype != np.int32:
        raise ValueError(f"crop params: hw int32 [N,2] with N >= 1 expected, got {hw.dtype} {hw.shape}")
    p = params.astype(np.int64)
    idx, top, left, flip = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    bad = (idx < 0) | (idx >= hw.shape[0])
    h, w = hw[np.where(bad, 0, idx)].astype(np.int64).T
    bad |= (top < 0) | (top > h - size) | (left < 0) | (left > w - size) | (flip < 0) | (flip > 1)
    if bad.any():
        b = int(np.argmax(bad))
        dims = "no such image" if not 0 <= idx[b] < hw.shape[0] else f"image {h[b]} x {w[b]}"
        raise ValueError(f"crop params: row {b} = (index {idx[b]}, top {top[b]}, left {left[b]}, flip {flip[b]}) is out of range for a "
                         f"{size} x {size} crop ({dims}, {hw.shape[0]} images)")


_norm_tables = {}


def normalize_table(device=None):
    """f32 [256]: `xmc_gan.dataset.to_normalized_tensor` of the bytes 0..255, computed by that function on the host (once) and, with a
    ``device``, uploaded (once per device): what `crop_flip_normalize` looks pixels up in"""
    if "host" not in _norm_tables:
        from xmc_gan.dataset import to_normalized_tensor
        _norm_tables["host"] = to_normalized_tensor(np.arange(256, dtype=np.uint8).reshape(16, 16)).reshape(256).contiguous()
    if device is None:
        return _norm_tables["host"]
    key = str(torch.device(device))
    if key not in _norm_tables:
        _norm_tables[key] = _norm_tables["host"].to(device)
    return _norm_tables[key]


def crop_flip_normalize(pool, offsets, hw, params, size, out=None, table=None):
    """B crops out of a device-resident pool of uint8 RGB HWC images -> f32 NCHW [B,3,size,size], the `imgs` of a training step:
    out[b,c,y,x] = table[pool[offsets[i] + ((top + y) * w + left + (flip ? size-1-x : x)) * 3 + c]] with (i, top, left, flip) = params[b].

    ``pool`` uint8 [bytes] (16-byte aligned, a multiple of 16 bytes), ``offsets`` int64 [N], both on the device; ``hw`` a `HostMirror` of
    int32 [N,2] (height, width); ``params`` a `HostMirror` of int32 [B,4], or the host array (uploaded here).  ``table``: f32 [256] on the
    device (default: `normalize_table`).  The host copies are checked (`validate_crop_params`) BEFORE anything is launched; a violation
    is a ValueError.  One launch on the current stream into a new tensor or the caller's ``out``.  size % 8 == 0."""
    if not isinstance(hw, HostMirror):
        raise TypeError("crop_flip_normalize: hw must be an ops.HostMirror (the bounds are checked on its host copy)")
    _need_cuda(pool, offsets, hw.dev)
    if not isinstance(params, HostMirror):
        if torch.is_tensor(params) and params.is_cuda:
            raise TypeError("crop_flip_normalize: params must come with their host copy (an ops.HostMirror or a host array)")
        host = params.numpy() if torch.is_tensor(params) else np.asarray(params)
        validate_crop_params(host, hw.host, int(size))
        params = HostMirror(host, pool.device)
    else:
        validate_crop_params(params.host, hw.host, int(size))
    size, N, B = int(size), hw.host.shape[0], params.host.shape[0]
    if pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise ValueError(f"crop_flip_normalize: pool must be a contiguous uint8 vector, got {pool.dtype} {tuple(pool.shape)}")
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (N,) or not offsets.is_contiguous():
        raise ValueError(f"crop_flip_normalize: offsets int64 [{N}] expected, got {offsets.dtype} {tuple(offsets.shape)}")
    if hw.dev.dtype != torch.int32 or params.dev.dtype != torch.int32 or tuple(params.dev.shape) != (B, 4) or tuple(hw.dev.shape) != (N, 2):
        raise ValueError("crop_flip_normalize: the device copies of hw / params do not match their host copies")
    table = normalize_table(pool.device) if table is None else table
    _need_cuda(table, params.dev)
    if table.dtype != torch.float32 or table.numel() != 256 or not table.is_contiguous():
        raise ValueError("crop_flip_normalize: table must be a contiguous f32 [256]")
    shape = (B, 3, size, size)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pool.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != pool.device:
        raise ValueError(f"crop_flip_normalize: out must be a contiguous f32 {shape} tensor on {pool.device}")
    L.call("xmc_crop_flip_normalize", _p(pool), pool.numel(), _p(offsets), _p(hw.dev), N, _p(params.dev), _p(table), _p(out), B, size, _st())
    return out


# ------------------------------------------------------------------------------------------ a batch's text-encoder outputs from cached embeddings (csrc/captionfeed.hip)
def validate_caption_rows(rows, n):
    """The bound `caption_gather` needs, checked on the host array: rows int32 [B], B >= 1, every entry in [0, n).  ValueError names the
    first offending entry."""
    rows = np.asarray(rows)
    if rows.ndim != 1 or rows.shape[0] < 1 or rows.dtype != np.int32:
        raise ValueError(f"caption rows: int32 [B] with B >= 1 expected, got {rows.dtype} {rows.shape}")
    bad = (rows < 0) | (rows >= n)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f"caption rows: entry {b} = {int(rows[b])} is out of range for a table of {n} captions")


def caption_gather(sent_tab, tok_tab, tok_offsets, lens, rows, T, out=None):
    """What a frozen text encoder returned for the captions ``rows`` when the tables were written: (words_embs f32 [B,E,T], sent_embs f32
    [B,E], mask bool [B,T], True at padding), one launch on the current stream.  words_embs[b,e,t] = tok_tab[tok_offsets[r] + t, e] for
    t < lens[r] and 0 beyond, sent_embs[b] = sent_tab[r], r = rows[b].

    ``sent_tab`` f32 [N,E], ``tok_tab`` f32 [rows,E] (only the valid tokens, caption by caption), ``tok_offsets`` int64 [N], ``lens`` int32 [N],
    all on the device; ``rows`` a `HostMirror` of int32 [B], or the host array (uploaded here).  The host copy is checked
    (`validate_caption_rows`) BEFORE anything is launched; a violation, or rows that come without a host copy, is a ValueError.  ``out``: the
    caller's three tensors.  E % 4 == 0, 1 <= T <= 64: anything else is the library's XMC_ESHAPE, raised as ValueError."""
    N = int(lens.shape[0]) if lens.dim() == 1 else -1
    if isinstance(rows, HostMirror):
        validate_caption_rows(rows.host, N)
    else:
        if torch.is_tensor(rows):
            if rows.device.type != "cpu":
                raise ValueError("caption_gather: rows must come with their host copy (an ops.HostMirror or a host array): the bound is "
                                 "checked there, without a read-back")
            rows = rows.numpy()
        validate_caption_rows(rows, N)
        _need_cuda(sent_tab)
        rows = HostMirror(rows, sent_tab.device)
    _need_cuda(sent_tab, tok_tab, tok_offsets, lens, rows.dev)
    T, B = int(T), rows.host.shape[0]
    if sent_tab.dtype != torch.float32 or sent_tab.dim() != 2 or sent_tab.shape[0] != N or not sent_tab.is_contiguous():
        raise ValueError(f"caption_gather: sent_tab must be a contiguous f32 [{N},E] tensor, got {sent_tab.dtype} {tuple(sent_tab.shape)}")
    E = int(sent_tab.shape[1])
    if tok_tab.dtype != torch.float32 or tok_tab.dim() != 2 or tok_tab.shape[1] != E or tok_tab.shape[0] < 1 or not tok_tab.is_contiguous():
        raise ValueError(f"caption_gather: tok_tab must be a contiguous f32 [rows >= 1,{E}] tensor, got {tok_tab.dtype} {tuple(tok_tab.shape)}")
    if tok_offsets.dtype != torch.int64 or tuple(tok_offsets.shape) != (N,) or not tok_offsets.is_contiguous() or lens.dtype != torch.int32 \
            or not lens.is_contiguous():
        raise ValueError(f"caption_gather: tok_offsets int64 [{N}] and lens int32 [{N}] expected, got {tok_offsets.dtype} "
                         f"{tuple(tok_offsets.shape)} and {lens.dtype} {tuple(lens.shape)}")
    if rows.dev.dtype != torch.int32 or tuple(rows.dev.shape) != (B,) or not rows.dev.is_contiguous():
        raise ValueError("caption_gather: the device copy of rows does not match its host copy")
    dev = sent_tab.device
    shapes = ((B, E, T), (B, E), (B, T))
    dtypes = (torch.float32, torch.float32, torch.bool)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    elif len(out) != 3 or any(tuple(o.shape) != s or o.dtype != d or not o.is_contiguous() or o.device != dev for o, s, d in zip(out, shapes, dtypes)):
        raise ValueError(f"caption_gather: out must be contiguous f32 {shapes[0]}, f32 {shapes[1]} and bool {shapes[2]} tensors on {dev}")
    words, sent, mask = out
    rc = getattr(L.load(), "xmc_caption_gather")(_p(sent_tab), _p(tok_tab), tok_tab.shape[0], _p(tok_offsets), _p(lens), N, _p(rows.dev), B, E, T,
                                                 _p(words), _p(sent), _p(mask), _st())
    if rc == -3:
        raise ValueError(f"caption_gather: XMC_ESHAPE (shape out of range): E = {E} must be a multiple of 4 and T = {T} in [1, 64]")
    L.check(rc, "xmc_caption_gather")
    return words, sent, mask


# ------------------------------------------------------------------------------------------ FID evaluation (csrc/fid.hip): f32, outside autograd
def _fid_arg(x, what, dtype, dims):
    _need_cuda(x)
    if x.dim() != dims or x.dtype != dtype or x.requires_grad:
        raise ValueError(f"{what}: a {dims}-d {dtype} tensor without a gradient expected, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def fid_resize_u8(u8, out_hw=None):
    """uint8 [N,H,W,3] (what `image_to_u8` writes and PIL reads) -> f32 engine image [N,OH,OW,8]: bilinear (align_corners=False, no
    antialias) to ``out_hw`` (None: the size it has), then 2 * (x / 255) - 1; channels 3..7 are zero"""
    u8 = _fid_arg(u8, "fid_resize_u8", torch.uint8, 4)
    N, H, W, c = u8.shape
    if c != 3 or N < 1 or H < 1 or W < 1:
        raise ValueError(f"fid_resize_u8: uint8 [N,H,W,3] expected, got {tuple(u8.shape)}")
    OH, OW = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if OH < 1 or OW < 1:
        raise ValueError(f"fid_resize_u8: output size {OH}x{OW}")
    y = torch.empty((N, OH, OW, 8), dtype=torch.float32, device=u8.device)
    L.call("xmc_fid_resize_u8", _p(u8), _p(y), N, H, W, OH, OW, _st())
    return y


_POOL_MODES = {"max": L.POOL_MAX, "avg": L.POOL_AVG_VALID, "avg_pad": L.POOL_AVG_PAD}


def resize_bilinear_f32(x, out_hw=None):
    """f32 NCHW [N,3,H,W] (what a generator returns) -> f32 engine image [N,OH,OW,8]: bilinear (align_corners=False, no antialias) to
    ``out_hw`` (None: the size it has) by `fid_resize_u8`'s coordinate rule, values not rescaled; channels 3..7 are zero"""
    x = _fid_arg(x, "resize_bilinear_f32", torch.float32, 4)
    N, c, H, W = x.shape
    if c != 3 or N < 1 or H < 1 or W < 1:
        raise ValueError(f"resize_bilinear_f32: f32 [N,3,H,W] expected, got {tuple(x.shape)}")
    OH, OW = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if OH < 1 or OW < 1:
        raise ValueError(f"resize_bilinear_f32: output size {OH}x{OW}")
    y = torch.empty((N, OH, OW, 8), dtype=torch.float32, device=x.device)
    L.call("xmc_resize_bilinear_f32", _p(x), _p(y), N, H, W, OH, OW, _st())
    return y


def pool3x3(x, mode, stride):
    """3x3 pool of f32 [N,H,W,C] (C % 4 == 0).  ``mode`` 'max', 'avg' (the sum over the window's in-image pixels divided by their number:
    avg_pool2d(count_include_pad=False)) or 'avg_pad' (the same sum / 9: count_include_pad=True; stride 1 only); ``stride`` 1 (padding 1,
    same size) or 2 (no padding, floor((H - 3) / 2) + 1 rows)"""
    x = _fid_arg(x, "pool3x3", torch.float32, 4)
    if mode not in _POOL_MODES or stride not in (1, 2) or (mode == "avg_pad" and stride != 1):
        raise ValueError(f"pool3x3: mode {mode!r}, stride {stride}")
    N, H, W, Cc = x.shape
    if N < 1 or Cc < 4 or Cc % 4 or H < 1 or W < 1 or (stride == 2 and (H < 3 or W < 3)):
        raise ValueError(f"pool3x3: {tuple(x.shape)} at stride {stride} (C % 4 == 0; stride 2 needs a whole 3x3 window)")
    OH, OW = (H, W) if stride == 1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    y = torch.empty((N, OH, OW, Cc), dtype=torch.float32, device=x.device)
    L.call("xmc_pool3x3", _p(x), _p(y), N, H, W, Cc, _POOL_MODES[mode], stride, _st())
    return y


def fid_moments(feats, total, outer):
    """total f64 [D] += column sums of feats f32 [B,D]; outer f64 [D,D] += feats^T feats, in f64 and in a fixed order (same bytes every run)"""
    feats = _fid_arg(feats, "fid_moments", torch.float32, 2)
    B, D = feats.shape
    for t, shape in ((total, (D,)), (outer, (D, D))):
        _need_cuda(t)
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != feats.device:
            raise ValueError(f"fid_moments: accumulator {tuple(t.shape)} {t.dtype}, a contiguous f64 {shape} on {feats.device} expected")
    if B < 1:
        raise ValueError("fid_moments: an empty batch")
    L.call("xmc_fid_moments", _p(feats), _p(total), _p(outer), B, D, _st())


# ------------------------------------------------------------------------------------------ R-precision (csrc/retrieval.hip): f32, outside autograd
def rprecision(img, txt, cand, return_scores=False):
    """Caption retrieval among K candidates per image: img f32 [N,D] image codes, txt f32 [M,D] caption codes, cand int32 [N,K] rows of
    ``txt`` (column 0: the image's own caption) -> rank int32 [N], the number of other candidates whose cosine beats the own caption's
    (0: a hit; K: the own caption scored NaN); ``return_scores``: (rank, score f32 [N,K]).  D % 4 == 0, D <= 1024.  ``cand`` is checked
    against [0, M) here, on the host (one synchronising reduction when it lives on the device)."""
    img, txt = _fid_arg(img, "rprecision", torch.float32, 2), _fid_arg(txt, "rprecision", torch.float32, 2)
    cand = torch.as_tensor(cand)
    if cand.dim() != 2 or cand.dtype != torch.int32:
        raise ValueError(f"rprecision: cand int32 [N,K] expected, got {cand.dtype} {tuple(cand.shape)}")
    (N, D), (M, D2), K = img.shape, txt.shape, cand.shape[1]
    if D != D2 or cand.shape[0] != N or N < 1 or M < 1 or K < 1 or txt.device != img.device:
        raise ValueError(f"rprecision: img {tuple(img.shape)}, txt {tuple(txt.shape)}, cand {tuple(cand.shape)} do not fit")
    if D % 4 or D > 1024:
        raise ValueError(f"rprecision: D = {D}; D % 4 == 0 and D <= 1024 expected")
    lo, hi = int(cand.min()), int(cand.max())
    if lo < 0 or hi >= M:
        raise ValueError(f"rprecision: candidate indices span [{lo}, {hi}], txt has {M} rows")
    cand = cand.to(img.device).contiguous()
    rank = torch.empty((N,), dtype=torch.int32, device=img.device)
    score = torch.empty((N, K), dtype=torch.float32, device=img.device) if return_scores else None
    L.call("xmc_rprecision", _p(img), _p(txt), _p(cand), _p(rank), _p(score), N, M, K, D, _st())
    return (rank, score) if return_scores else rank


# ------------------------------------------------------------------------------------------ precision / recall / density / coverage (csrc/manifold.hip): f32, outside autograd
def _manifold_dims(what, *xs):
    D = xs[0].shape[1]
    if any(x.shape[1] != D or x.shape[0] < 1 or x.device != xs[0].device for x in xs) or D < 4 or D % 4 or D > 4096:
        raise ValueError(f"{what}: f32 [N,D] rows on one device with D % 4 == 0 and 4 <= D <= 4096 expected, got {[tuple(x.shape) for x in xs]}")
    return D


def _manifold_slices(what, nq, nc, slices):
    slices = int(slices)
    if slices < 0:
        raise ValueError(f"{what}: slices = {slices}")
    return getattr(L.load(), "xmc_manifold_slices")(nq, nc, slices)


def row_sqnorm(x):
    """|x_i|^2 of the rows of x f32 [N,D] (D % 4 == 0, D <= 4096) -> f32 [N], summed in a fixed order"""
    x = _fid_arg(x, "row_sqnorm", torch.float32, 2)
    D = _manifold_dims("row_sqnorm", x)
    n2 = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    L.call("xmc_row_sqnorm", _p(x), _p(n2), x.shape[0], D, _st())
    return n2


def knn_radius2(x, k, slices=0):
    """rad2 f32 [N]: the k-th smallest squared distance from row i of x f32 [N,D] to the OTHER rows (excluded by index; duplicates are
    neighbours at distance 0).  1 <= k <= 16, N >= k + 1.  ``slices``: ranges the candidate rows are split into (0: the library
    chooses); the result is the same bytes for every value."""
    x = _fid_arg(x, "knn_radius2", torch.float32, 2)
    D, N, k = _manifold_dims("knn_radius2", x), x.shape[0], int(k)
    if not 1 <= k <= 16 or N < k + 1:
        raise ValueError(f"knn_radius2: k = {k} with {N} rows; 1 <= k <= 16 and N >= k + 1 expected")
    S = _manifold_slices("knn_radius2", N, N, slices)
    n2 = row_sqnorm(x)
    r2 = torch.empty((N,), dtype=torch.float32, device=x.device)
    ws = torch.empty((S * N * k,), dtype=torch.float32, device=x.device) if S > 1 else None
    L.call("xmc_knn_radius2", _p(x), _p(n2), _p(r2), _p(ws), 0 if ws is None else ws.numel() * 4, N, D, k, S, _st())
    return r2


def manifold_count(a, b, rb2, slices=0):
    """For every row i of a f32 [Na,D] against the rows of b f32 [Nb,D]: count int32 [Na] = the number of rows j of b with
    |a_i - b_j|^2 <= rb2[j] (rb2 f32 [Nb], e.g. `knn_radius2(b, k)`), and near2 f32 [Na] = min_j |a_i - b_j|^2.  ``rb2`` None: count is
    None and only near2 is computed.  Returns (count, near2); the same bytes for every ``slices``."""
    a, b = _fid_arg(a, "manifold_count", torch.float32, 2), _fid_arg(b, "manifold_count", torch.float32, 2)
    D, Na, Nb = _manifold_dims("manifold_count", a, b), a.shape[0], b.shape[0]
    if rb2 is not None:
        rb2 = _fid_arg(rb2, "manifold_count", torch.float32, 1)
        if rb2.shape[0] != Nb or rb2.device != a.device:
            raise ValueError(f"manifold_count: rb2 {tuple(rb2.shape)} on {rb2.device}, f32 [{Nb}] on {a.device} expected")
    S = _manifold_slices("manifold_count", Na, Nb, slices)
    na2, nb2 = row_sqnorm(a), row_sqnorm(b)
    count = torch.empty((Na,), dtype=torch.int32, device=a.device) if rb2 is not None else None
    near2 = torch.empty((Na,), dtype=torch.float32, device=a.device)
    ws = torch.empty((S * Na * 2,), dtype=torch.float32, device=a.device) if S > 1 else None
    L.call("xmc_manifold_count", _p(a), _p(na2), _p(b), _p(nb2), _p(rb2), _p(count), _p(near2), _p(ws), 0 if ws is None else ws.numel() * 4,
           Na, Nb, D, S, _st())
    return count, near2


# ------------------------------------------------------------------------------------------ KID / Inception Score (csrc/kid.hip): outside autograd
def _index_table(what, idx, n, device):
    """an int32 [S,m] table of rows of a bank of ``n`` rows, checked against [0, n) HERE, on the host, before anything is launched"""
    idx = torch.as_tensor(idx)
    if idx.dim() != 2 or idx.dtype != torch.int32 or idx.shape[0] < 1:
        raise ValueError(f"{what}: an int32 [S,m] index table expected, got {idx.dtype} {tuple(idx.shape)}")
    if idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n:
            raise ValueError(f"{what}: the indices span [{lo}, {hi}], the bank has {n} rows")
    return idx.to(device).contiguous()


def poly_mmd_sums(real, fake, idx_real, idx_fake):
    """The kernel sums of KID's unbiased MMD^2, k(x, y) = (x.y / D + 1)^3, for S subsets of m rows per side in one launch: real f32 [Nr,D],
    fake f32 [Nf,D], idx_real / idx_fake int32 [S,m] (rows of the banks, checked against them on the host) -> f64 [S,3]: the sum of k over
    the ordered pairs i != j (by POSITION in the subset) of the real subset, the same of the generated one, and the sum over all m^2 cross
    pairs.  D % 4 == 0, 4 <= D <= 4096, m >= 2.  No m x m matrix and no gathered copy of a subset is stored; the same bytes every run."""
    real, fake = _fid_arg(real, "poly_mmd_sums", torch.float32, 2), _fid_arg(fake, "poly_mmd_sums", torch.float32, 2)
    D = _manifold_dims("poly_mmd_sums", real, fake)
    ir, jf = _index_table("poly_mmd_sums", idx_real, real.shape[0], real.device), _index_table("poly_mmd_sums", idx_fake, fake.shape[0], real.device)
    (S, m) = ir.shape
    if tuple(jf.shape) != (S, m) or m < 2 or S > 65535:
        raise ValueError(f"poly_mmd_sums: index tables {tuple(ir.shape)} and {tuple(jf.shape)}; two [S,m] tables with m >= 2 and S <= 65535 expected")
    tiles = getattr(L.load(), "xmc_poly_mmd_tiles")(m)
    out = torch.empty((S, 3), dtype=torch.float64, device=real.device)
    ws = torch.empty((S * tiles,), dtype=torch.float64, device=real.device)
    L.call("xmc_poly_mmd_sums", _p(real), _p(fake), _p(ir), _p(jf), _p(out), _p(ws), ws.numel() * 8, real.shape[0], fake.shape[0], D, S, m, _st())
    return out


def inception_score_sums(logits, splits, classes=None):
    """logits f32 [N,ld] (``classes``: only the first that many columns are logits, the others are never read) cut into ``splits``
    consecutive parts [s N // splits, (s + 1) N // splits) -> (H f64 [splits], P f64 [splits,C]): per part the sum of p log p over rows and
    classes and the per-class sum of p over rows, p = softmax(row), everything in f64 and in a fixed order.  C <= 1024, 1 <= splits <= N."""
    _need_cuda(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.requires_grad or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise ValueError(f"inception_score_sums: f32 logits [N,C] with unit column stride expected, got {logits.dtype} {tuple(logits.shape)}")
    N, C, splits = logits.shape[0], int(logits.shape[1] if classes is None else classes), int(splits)
    if not 1 <= C <= min(1024, logits.shape[1]) or not 1 <= splits <= min(N, 65535):
        raise ValueError(f"inception_score_sums: {N} rows, {C} of {logits.shape[1]} columns, {splits} splits; 1 <= C <= 1024 and 1 <= splits <= N expected")
    H = torch.empty((splits,), dtype=torch.float64, device=logits.device)
    P = torch.empty((splits, C), dtype=torch.float64, device=logits.device)
    nbytes = getattr(L.load(), "xmc_inception_score_ws_bytes")(N, C, splits)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=logits.device)
    L.call("xmc_inception_score", _p(logits), logits.stride(0), _p(H), _p(P), _p(ws), nbytes, N, C, splits, _st())
    return H, P


# ------------------------------------------------------------------------------------------ text front end
def embedding(ids, table):
    """nn.Embedding lookup (encoder.py:132), forward only (the encoder is frozen, train_gan.py:466-468).
    ids: int64 [...] on the device; table f32 [V, D] with D % 4 == 0.  Returns f32 [..., D]."""
    if not table.is_cuda or not ids.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.embedding: CPU tensors are not supported (no CPU fallback)")
    assert ids.dtype == torch.int64 and table.dtype == torch.float32 and table.dim() == 2
    ids = ids.contiguous()
    table = table.detach().contiguous()
    out = torch.empty(*ids.shape, table.shape[1], dtype=torch.float32, device=table.device)
    L.call("xmc_embedding_gather", _p(ids), _p(table), _p(out), ids.numel(), table.shape[1], table.shape[0], _st())
    return out


def lstm_bidir(xproj, w_hh, lens, T):
    """One-layer bidirectional LSTM recurrence over length-packed sequences (encoder.py:134-147), forward only.
    xproj f32 [B,T,2,4H] (input projections + both biases), w_hh f32 [2,4H,H], lens int32 [B].
    Returns words [B,2H,T] (zero at t >= len) and sent [B,2H] = [h_fwd(len-1), h_rev(0)]."""
    if not xproj.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.lstm_bidir: CPU tensors are not supported (no CPU fallback)")
    B, H = xproj.shape[0], w_hh.shape[2]
    assert xproj.dtype == torch.float32 and xproj.is_contiguous() and xproj.shape == (B, T, 2, 4 * H)
    assert w_hh.dtype == torch.float32 and w_hh.is_contiguous() and w_hh.shape == (2, 4 * H, H)
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B
    words = torch.empty(B, 2 * H, T, dtype=torch.float32, device=xproj.device)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=xproj.device)
    L.call("xmc_lstm_bidir", _p(xproj), _p(w_hh), _p(lens), _p(words), _p(sent), B, T, H, _st())
    return words, sent


def gru_bidir(xproj, w_hh, b_hn, lens, T):
    """One-layer bidirectional GRU recurrence over length-packed sequences (encoder.py:99-102,134-147 with RNN_TYPE 'GRU'),
    forward only.  xproj f32 [B,T,2,3H] (W_i* x + b_i*, plus b_h* for the r and z rows), w_hh f32 [2,3H,H], b_hn f32 [2,H],
    lens int32 [B].  Returns words [B,2H,T] (zero at t >= len) and sent [B,2H] = [h_fwd(len-1), h_rev(0)]."""
    if not xproj.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.gru_bidir: CPU tensors are not supported (no CPU fallback)")
    B, H = xproj.shape[0], w_hh.shape[2]
    assert xproj.dtype == torch.float32 and xproj.is_contiguous() and xproj.shape == (B, T, 2, 3 * H)
    assert w_hh.dtype == torch.float32 and w_hh.is_contiguous() and w_hh.shape == (2, 3 * H, H)
    assert b_hn.dtype == torch.float32 and b_hn.is_contiguous() and b_hn.shape == (2, H)
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B
    words = torch.empty(B, 2 * H, T, dtype=torch.float32, device=xproj.device)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=xproj.device)
    L.call("xmc_gru_bidir", _p(xproj), _p(w_hh), _p(b_hn), _p(lens), _p(words), _p(sent), B, T, H, _st())
    return words, sent


# sentence encoder (SBERT_ENCODER: a frozen RoBERTa forward; csrc/transformer.hip).  Forward only, like the RNN front end above; the GEMMs
# between these go through `linear`.  `out16`: also return the result in that 16-bit dtype (the next GEMM's operand), None in fp32 mode.
# The limits of the kernels that this encoder and CLIP's towers share (csrc/encoder_kernels.h), for the classes that check a model against them:
ATTENTION_MAX_T = 64        # longest sequence of the attention kernel (AT_T); its head dimension is 64 as well
LN_MAX_WIDTH = 1024         # widest row of the LayerNorm kernels (64 lanes x LN_MAXU 16-byte units), a multiple of 64


def _enc_f32c(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "f32 contiguous tensors expected"


def _enc_out16(like, out16):
    assert out16 in (None, torch.float32) or _code(out16) == L.H16
    return None if out16 in (None, torch.float32) else torch.empty_like(like, dtype=out16)


def roberta_embed_ln(ids, lens, word, pos, type0, gamma, beta, eps, pad_idx, out16=None):
    """RobertaEmbeddings: LN(word[ids] + token_type[0] + position[p]) with p = cumsum(mask) * mask + pad_idx computed in the kernel from
    the lengths of the right-padded batch.  ids int64 [B,T], lens int32 [B]; word [V,H], pos [P,H], type0 [H].
    Returns f32 [B*T,H] (and its 16-bit copy when `out16` names one, else None)."""
    if not ids.is_cuda or not word.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.roberta_embed_ln: CPU tensors are not supported (no CPU fallback)")
    B, T = ids.shape
    H = word.shape[1]
    assert ids.dtype == torch.int64 and ids.is_contiguous() and lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B
    _enc_f32c(word, pos, type0, gamma, beta)
    assert pos.shape[1] == H and type0.numel() == H and gamma.numel() == H and beta.numel() == H
    out = torch.empty(B * T, H, dtype=torch.float32, device=word.device)
    o16 = _enc_out16(out, out16)
    L.call("xmc_roberta_embed_ln", _p(ids), _p(lens), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), _p(out), _p(o16), B, T, H,
           word.shape[0], pos.shape[0], int(pad_idx), float(eps), _st())
    return out, o16


def add_layernorm(x, res, gamma, beta, eps, bias=None, out16=None):
    """LN(x [+ bias] [+ res]) * gamma + beta over the last dimension of f32 [rows,H] (H a multiple of 64, <= 1024): one wave per row, f32
    two-pass statistics.  Returns f32 [rows,H] and its 16-bit copy (None unless `out16` names a 16-bit dtype)."""
    if not x.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.add_layernorm: CPU tensors are not supported (no CPU fallback)")
    rows, H = x.shape
    _enc_f32c(x, res, gamma, beta, bias)
    assert res is None or res.shape == x.shape
    assert gamma.numel() == H and beta.numel() == H and (bias is None or bias.numel() == H)
    out = torch.empty_like(x)
    o16 = _enc_out16(out, out16)
    L.call("xmc_add_layernorm", _p(x), _p(bias), _p(res), _p(gamma), _p(beta), _p(out), _p(o16), rows, H, float(eps), _st())
    return out, o16


def _attention(name, qkv, lens, B, T, heads, out_dtype):
    """`attention_short` (``lens`` int32 [B]) and `attention_causal` (``lens`` None): the checks, the output, the launch"""
    if not qkv.is_cuda:
        raise RuntimeError(f"xmc_gan_amd.ops.{name}: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(qkv)
    assert qkv.dim() == 2 and qkv.shape[0] == B * T and qkv.shape[1] % (3 * heads) == 0
    d = qkv.shape[1] // (3 * heads)
    assert d == 64 and 1 <= T <= ATTENTION_MAX_T, f"{name} is built for head dimension 64 and T <= 64, got d={d}, T={T}"
    assert lens is None or (lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B)
    out = torch.empty(B * T, heads * d, dtype=out_dtype, device=qkv.device)
    if lens is None:
        L.call("xmc_attention_causal", _p(qkv), _p(out), B, T, heads, d, _st())
    else:
        L.call("xmc_attention_short", _p(qkv), _p(lens), _p(out), B, T, heads, d, _code(out_dtype), _st())
    return out


def attention_short(qkv, lens, B, T, heads, out_dtype=torch.float32):
    """softmax(Q K^T / sqrt(d) + key padding mask) V per (sample, head) from the fused QKV projection f32 [B*T,3H] (rows [Q | K | V]), for
    head dimension 64 and T <= 64; the scores never reach memory.  Rows of padded queries come back as zeros.  Returns [B*T,H]."""
    assert lens is not None
    return _attention("attention_short", qkv, lens, B, T, heads, out_dtype)


def _bias_act(name, x, bias, out_dtype):
    """`bias_gelu` and `bias_quick_gelu` (f32 only: its entry point takes no dtype): the checks, the output, the launch"""
    if not x.is_cuda:
        raise RuntimeError(f"xmc_gan_amd.ops.{name}: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(x, bias)
    assert x.dim() == 2 and bias.numel() == x.shape[1]
    out = torch.empty_like(x, dtype=out_dtype)
    dt = () if name == "bias_quick_gelu" else (_code(out_dtype),)
    L.call("xmc_" + name, _p(x), _p(bias), _p(out), x.shape[0], x.shape[1], *dt, _st())
    return out


def bias_gelu(x, bias, out_dtype=torch.float32):
    """gelu(x + bias) with the exact (erf) GELU -- Hugging Face's hidden_act "gelu" -- over f32 [rows,F], F % 8 == 0."""
    return _bias_act("bias_gelu", x, bias, out_dtype)


def sbert_pool(hidden, lens, max_length, normalize):
    """The tail of SBERT_ENCODER.forward (encoder.py:50-70) in one launch.  hidden f32 [B,T,H], lens int32 [B], T <= max_length <= 64.
    Returns words_embs [B,H,max_length] (token embeddings x attention mask, zero at padding and beyond T), sent_embs [B,H] (mean over the
    valid tokens, L2-normalised when `normalize`) and mask bool [B,max_length] (True at padding)."""
    if not hidden.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.sbert_pool: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(hidden)
    B, T, H = hidden.shape
    assert T <= max_length <= 64, f"sbert_pool is built for T <= max_length <= 64, got T={T}, max_length={max_length}"
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B
    words = torch.empty(B, H, max_length, dtype=torch.float32, device=hidden.device)
    sent = torch.empty(B, H, dtype=torch.float32, device=hidden.device)
    mask = torch.empty(B, max_length, dtype=torch.bool, device=hidden.device)
    L.call("xmc_sbert_pool", _p(hidden), _p(lens), _p(words), _p(sent), _p(mask), B, T, H, max_length, int(bool(normalize)), _st())
    return words, sent, mask


# CLIPScore (xmc_gan_amd.clip: the CLIP ViT-B/32 towers; csrc/clip.hip).  Forward only and f32 in every precision mode; the GEMMs between
# these go through `_conv_fwd_raw`, whose epilogue adds the bias and the residual.
_pil_tables = {}          # (in, out) -> (bounds, coeffs, ksize) on the host;  (in, out, device) -> the same as int32 device tensors


def _pil_cubic(x):
    """Pillow's bicubic_filter: the Keys cubic with a = -0.5"""
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def pil_bicubic_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis of ``n_in`` -> ``n_out`` samples, in f64 in Pillow's
    order of operations: (bounds [(first sample, count)] * n_out, coeffs [[int] * ksize] * n_out, ksize).  The weights carry 22 fraction
    bits; refuses a table whose worst case 255 * sum |k| + 2^21 does not fit the kernels' int32 accumulator."""
    key = (int(n_in), int(n_out))
    if key not in _pil_tables:
        n_in, n_out = key
        assert n_in >= 1 and n_out >= 1
        scale = n_in / n_out
        fscale = scale if scale > 1.0 else 1.0
        support = 2.0 * fscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fscale
        bounds, coeffs = [], []
        for xx in range(n_out):
            center = 0.0 + (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), n_in) - xmin
            w = [_pil_cubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            k = [int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0) for v in w] + [0] * (ksize - xmax)
            if 255 * sum(abs(v) for v in k) + (1 << 21) >= 1 << 31:
                raise ValueError(f"resize_bicubic_u8: the {n_in} -> {n_out} filter overflows the int32 accumulator")
            bounds.append((xmin, xmax))
            coeffs.append(k)
        _pil_tables[key] = (bounds, coeffs, ksize)
    return _pil_tables[key]


def _pil_tables_dev(n_in, n_out, device):
    key = (int(n_in), int(n_out), str(device))
    if key not in _pil_tables:
        bounds, coeffs, ksize = pil_bicubic_tables(n_in, n_out)
        _pil_tables[key] = (torch.tensor(bounds, dtype=torch.int32).to(device).contiguous(),
                            torch.tensor(coeffs, dtype=torch.int32).to(device).contiguous(), ksize)
    return _pil_tables[key]


def _resize_u8_h(u8, ow):
    """the horizontal pass into uint8 [N,H,ow,3] (Pillow skips a pass that changes nothing; an identity filter gives the same bytes)"""
    if not u8.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.resize_bicubic_u8: CPU tensors are not supported (no CPU fallback)")
    assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[3] == 3 and u8.is_contiguous(), "uint8 [N,H,W,3] expected"
    N, H, W, _ = u8.shape
    if ow == W:
        return u8
    bw, cw, kw = _pil_tables_dev(W, ow, u8.device)
    mid = torch.empty(N, H, ow, 3, dtype=torch.uint8, device=u8.device)
    L.call("xmc_clip_resize_h_u8", _p(u8), _p(mid), _p(bw), _p(cw), N, H, W, ow, kw, _st())
    return mid


def resize_bicubic_u8(u8, oh, ow):
    """``PIL.Image.resize((ow, oh), BICUBIC)`` of uint8 [N,H,W,3] images, bit for bit: Pillow's antialiased two-pass integer resampling
    (horizontal into uint8, then vertical), with the coefficient tables computed on the host in f64.  Returns uint8 [N,oh,ow,3]."""
    mid = _resize_u8_h(u8, ow)
    N, H = mid.shape[:2]
    bh, ch, kh = _pil_tables_dev(H, oh, mid.device)
    out = torch.empty(N, oh, ow, 3, dtype=torch.uint8, device=mid.device)
    L.call("xmc_clip_resize_v_u8", _p(mid), _p(out), _p(bh), _p(ch), None, N, H, ow, oh, kh, 0, 0, 1, 0, 0, _st())
    return out


def clip_resize_target(h, w, short):
    """CLIP's resize: the short side to ``short``, the long side to int(short * long / short side)"""
    return (short, int(short * w / h)) if h <= w else (int(short * h / w), short)


def clip_patch_rows(u8, short, crop, patch, lut):
    """CLIP's image preprocessing in two launches: resize (short side ``short``, `resize_bicubic_u8`'s arithmetic), centre crop
    ``crop`` x ``crop``, per-channel normalisation through ``lut`` f32 [3,256], written as the patch embedding's GEMM operand
    f32 [N*(crop/patch)^2, 3*patch*patch] (column c*patch^2 + py*patch + px: the flatten order of ``patch_embedding.weight``)."""
    N, H, W, _ = u8.shape
    oh, ow = clip_resize_target(H, W, short)
    assert crop % patch == 0 and crop <= min(oh, ow), f"a {crop}-pixel crop of a {oh}x{ow} image in {patch}-pixel patches is not built"
    _enc_f32c(lut)
    assert tuple(lut.shape) == (3, 256)
    mid = _resize_u8_h(u8, ow)
    bh, ch, kh = _pil_tables_dev(H, oh, mid.device)
    g = crop // patch
    out = torch.empty(N * g * g, 3 * patch * patch, dtype=torch.float32, device=mid.device)
    L.call("xmc_clip_resize_v_u8", _p(mid), _p(out), _p(bh), _p(ch), _p(lut), N, H, ow, oh, kh, 1, crop, patch, (oh - crop) // 2,
           (ow - crop) // 2, _st())
    return out


def attention_causal(qkv, B, T, heads):
    """`attention_short` over keys j <= i (CLIP's text tower): qkv f32 [B*T,3H], head dimension 64, T <= 64.  Returns f32 [B*T,H]."""
    return _attention("attention_causal", qkv, None, B, T, heads, torch.float32)


ATTENTION_LONG_MAX_T = 1024     # longest sequence of `attention_long` (AL_MAX_T of csrc/attention_long.hip)


def attention_long(qkv, lens, B, T, heads, causal=False):
    """softmax(Q K^T / sqrt(64) + mask) V for 1 <= T <= 1024 on the exact-f32 MFMA, K and V streamed through LDS in 64-key tiles with a
    running maximum and sum (csrc/attention_long.hip): qkv f32 [B*T,3H] as `attention_short` takes it; query r of sample b sees keys
    j < lens[b] (int32 [B]; T when ``lens`` is None) and, with ``causal``, j <= r.  Rows of padded queries come back as zeros.
    A sample's bytes depend neither on T nor on the batch nor on what lies behind its length.  Returns f32 [B*T,H]."""
    if not qkv.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.attention_long: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(qkv)
    assert qkv.dim() == 2 and qkv.shape[0] == B * T and qkv.shape[1] % (3 * heads) == 0
    d = qkv.shape[1] // (3 * heads)
    assert d == 64 and 1 <= T <= ATTENTION_LONG_MAX_T, f"attention_long is built for head dimension 64 and T <= 1024, got d={d}, T={T}"
    assert lens is None or (lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == B and lens.is_cuda)
    out = torch.empty(B * T, heads * d, dtype=torch.float32, device=qkv.device)
    L.call("xmc_attention_long", _p(qkv), _p(lens), _p(out), B, T, heads, d, int(bool(causal)), _st())
    return out


def bias_quick_gelu(x, bias):
    """v * sigmoid(1.702 v), v = x + bias -- Hugging Face's hidden_act "quick_gelu" -- over f32 [rows,F], F % 8 == 0."""
    return _bias_act("bias_quick_gelu", x, bias, torch.float32)


def clip_vision_embed(patch, cls, pos, gamma, beta, eps):
    """CLIPVisionEmbeddings + pre_layrnorm: rows [class + pos[0] | patch[p] + pos[1 + p]] of every image, then LayerNorm.
    patch f32 [N*GG,W], cls [W], pos [GG+1,W].  Returns f32 [N*(GG+1),W]."""
    if not patch.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.clip_vision_embed: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(patch, cls, pos, gamma, beta)
    GG, W = pos.shape[0] - 1, pos.shape[1]
    assert patch.dim() == 2 and patch.shape[1] == W and GG >= 1 and patch.shape[0] % GG == 0
    assert cls.numel() == W and gamma.numel() == W and beta.numel() == W
    N = patch.shape[0] // GG
    out = torch.empty(N * (GG + 1), W, dtype=torch.float32, device=patch.device)
    L.call("xmc_clip_vision_embed", _p(patch), _p(cls), _p(pos), _p(gamma), _p(beta), _p(out), N, GG, W, float(eps), _st())
    return out


def clip_text_embed(ids, tok, pos):
    """CLIPTextEmbeddings: tok[ids] + pos[t].  ids int64 [B,T] on the device, tok [V,W], pos [P,W] with T <= P.  Returns f32 [B*T,W]."""
    if not ids.is_cuda or not tok.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.clip_text_embed: CPU tensors are not supported (no CPU fallback)")
    B, T = ids.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    _enc_f32c(tok, pos)
    assert pos.shape[1] == tok.shape[1] and T <= pos.shape[0]
    out = torch.empty(B * T, tok.shape[1], dtype=torch.float32, device=tok.device)
    L.call("xmc_clip_text_embed", _p(ids), _p(tok), _p(pos), _p(out), B, T, tok.shape[1], tok.shape[0], pos.shape[0], _st())
    return out


def clip_pool_ln(x, index, T, gamma, beta, eps):
    """LayerNorm of row index[b] of every sample of x f32 [B*T,W]; index int32 [B].  Returns f32 [B,W]."""
    if not x.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.clip_pool_ln: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(x, gamma, beta)
    B, W = index.numel(), x.shape[1]
    assert x.dim() == 2 and x.shape[0] == B * T and index.dtype == torch.int32 and index.is_contiguous()
    assert gamma.numel() == W and beta.numel() == W
    out = torch.empty(B, W, dtype=torch.float32, device=x.device)
    L.call("xmc_clip_pool_ln", _p(x), _p(index), _p(gamma), _p(beta), _p(out), B, T, W, float(eps), _st())
    return out


def clip_cosine(img, txt, caption_of_image=None):
    """per image, the cosine of its feature row img [N,D] and the row of its caption in txt [M,D]: row caption_of_image[n] (int32 [N]),
    or row n.  One wave per image, a fixed summation order.  Returns f32 [N]."""
    if not img.is_cuda or not txt.is_cuda:
        raise RuntimeError("xmc_gan_amd.ops.clip_cosine: CPU tensors are not supported (no CPU fallback)")
    _enc_f32c(img, txt)
    N, D = img.shape
    M = txt.shape[0]
    assert txt.shape[1] == D
    if caption_of_image is None:
        assert N <= M, "without caption_of_image every image needs a caption row of its own"
    else:
        assert caption_of_image.dtype == torch.int32 and caption_of_image.is_contiguous() and caption_of_image.numel() == N
    out = torch.empty(N, dtype=torch.float32, device=img.device)
    L.call("xmc_clip_cosine", _p(img), _p(txt), _p(caption_of_image), _p(out), N, M, D, _st())
    return out
