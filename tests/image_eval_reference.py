"""Float64 numpy yardstick of the image scores (permuto_sdf_amd/image_eval.py, csrc/image_eval.hip), written from their
definition; tests/test_image_eval_host.py pins it to a float64 transcription of piq's published formula, and
tests/test_gpu_image_eval.py compares the kernels with it.

Images are (N, C, H, W) arrays, float or uint8 (a uint8 value v stands for v / 255); the optional mask is (N, 1, H, W) (or
anything that broadcasts against the images) and multiplies both images; data_range divides both:
    value = element * mask / data_range.
PSNR = -10 log10(mse + 1e-8), mse over C H W of every image, masked pixels included.  SSIM: average pooling by
f = max(1, round(min(H, W) / 256)) (stride f, remainders dropped), a separable Gaussian window of `kernel_size` taps over valid
positions only, (2 mx my + c1) / (mx^2 + my^2 + c1) * (2 sxy + c2) / (sxx + syy + c2) with c1 = k1^2 and c2 = k2^2, mean over
the map and then over channels.  Every parameter is an argument."""
import numpy as np


def as_f64(img):
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def values(img, mask=None, data_range=1.0):
    x = as_f64(img)
    if mask is not None:
        x = x * as_f64(mask)
    return x / float(data_range)


def pooling_factor(H, W):
    return max(1, round(min(H, W) / 256))


def gaussian_weights(kernel_size=11, sigma=1.5):
    d = np.arange(kernel_size, dtype=np.float64) - (kernel_size - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    total = 0.0
    for v in g:                      # index order, as csrc/image_eval_plan.h adds them
        total += float(v)
    return g / total


def pool(x, f):
    if f <= 1:
        return x
    H, W = x.shape[-2:]
    h, w = H // f, W // f
    return x[..., :h * f, :w * f].reshape(*x.shape[:-2], h, f, w, f).mean(axis=(-3, -1))


def window(x, g):
    """the separable window over valid positions: rows, then columns"""
    k = len(g)
    H, W = x.shape[-2:]
    t = sum(g[i] * x[..., i:H - k + 1 + i, :] for i in range(k))
    return sum(g[j] * t[..., :, j:W - k + 1 + j] for j in range(k))


def sq_diff(pred, gt, mask=None, data_range=1.0):
    """-> [N]: sum over (c, h, w) of (x - y)^2"""
    d = values(pred, mask, data_range) - values(gt, mask, data_range)
    return (d * d).reshape(d.shape[0], -1).sum(axis=1)


def psnr(pred, gt, mask=None, data_range=1.0):
    """-> [N] dB"""
    x = values(pred, mask, data_range)
    mse = sq_diff(pred, gt, mask, data_range) / float(np.prod(x.shape[1:]))
    return -10.0 * np.log10(mse + 1e-8)


def ssim(pred, gt, mask=None, data_range=1.0, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True):
    """-> (score [N], map [N, C, h', w'])"""
    x, y = values(pred, mask, data_range), values(gt, mask, data_range)
    f = pooling_factor(*x.shape[-2:]) if downsample else 1
    x, y = pool(x, f), pool(y, f)
    if min(x.shape[-2:]) < kernel_size:
        raise ValueError("pooled image %s smaller than the window" % (x.shape[-2:],))
    g = gaussian_weights(kernel_size, kernel_sigma)
    c1, c2 = k1 * k1, k2 * k2
    mx, my = window(x, g), window(y, g)
    sxx, syy, sxy = window(x * x, g) - mx * mx, window(y * y, g) - my * my, window(x * y, g) - mx * my
    m = (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * (2.0 * sxy + c2) / (sxx + syy + c2)
    return m.mean(axis=(-1, -2)).mean(axis=-1), m


def to_u8(img):
    """clamp(rint(img * 255), 0, 255) as uint8, ties to even; the product is formed in the image's own precision"""
    img = np.asarray(img)
    return np.clip(np.rint(img * img.dtype.type(255)), 0, 255).astype(np.uint8)


def scene(N, C, H, W, seed):
    """a seeded 8-bit pair (pred, gt), uint8 (N, C, H, W): a smooth pattern, a block of exact zeros in both images (the masked
    region), a saturated flat block at 255, noise on the rest"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(xx / (5 + c) + n) * np.cos(yy / (7 + n)) for n in range(N) for c in range(C)])
    base = base.reshape(N, C, H, W)
    base[..., :H // 3, :W // 2] = 0.0
    base[..., H // 3:H // 2, W // 2:] = 1.0
    inside = (base > 0) & (base < 1)
    gt = np.clip(base + 0.02 * r.standard_normal(base.shape) * inside, 0, 1)
    pr = np.clip(gt + 0.05 * r.standard_normal(base.shape) * (base > 0), 0, 1)
    return to_u8(pr.astype(np.float32)), to_u8(gt.astype(np.float32))


def block_mask(N, H, W):
    """mask of zeros and ones as an 8-bit image, 0 / 255, (N, 1, H, W): zero over the scene's block of zeros and a strip beside it"""
    m = np.full((N, 1, H, W), 255, dtype=np.uint8)
    m[..., :H // 3 + 1, :W // 2 + 2] = 0
    return m


def graded_mask(N, H, W, seed):
    """float32 mask in [0, 1] with exact zeros and ones in it"""
    r = np.random.default_rng(seed)
    m = np.clip(r.uniform(-0.3, 1.3, (N, 1, H, W)), 0, 1).astype(np.float32)
    return m
