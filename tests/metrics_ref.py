"""Two independent restatements of the validation metrics mfnerf_image_metrics computes (the
reference's torchmetrics PSNR / SSIM, train.py:65-67, 198-237), and the seeded test images.

ssim64 / mse64: fp64 numpy, the definition as include/mfnerf.h states it -- the separable 11-tap
Gaussian of sigma 1.5 over the windows that lie inside the image, nothing padded.
ssim32_torchmetrics_form: fp32 torch in the form torchmetrics runs -- reflect pad 5, a depthwise
conv2d with the 11x11 outer-product kernel, the map cropped by 5, the mean.  That the two agree on
noise is the check that "pad, then crop" equals "valid windows"; where they part (flat and smooth
images) is fp32 cancellation in E[x^2] - mu^2, the reason the kernel accumulates in fp64.

Images are (H*W, 3) arrays, row-major pixels, rgb interleaved, values in [0, 1].
"""
import numpy as np

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def weights():
    """g[k] ~ exp(-(k-5)^2 / (2 sigma^2)), k = 0..10, normalised to sum 1 (fp64)."""
    k = np.arange(WINDOW, dtype=np.float64) - (WINDOW - 1) / 2
    e = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return e / e.sum()


def _filter_valid(a):
    """The separable window over (H, W, C) fp64 -> (H-10, W-10, C): valid windows only."""
    g = weights()
    H, W = a.shape[:2]
    h = sum(g[k] * a[:, k:k + W - WINDOW + 1] for k in range(WINDOW))
    return sum(g[k] * h[k:k + H - WINDOW + 1] for k in range(WINDOW))


def mse64(pred, target):
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return float(((p - t) ** 2).mean())


def ssim64(pred, target, H, W):
    p = np.asarray(pred, dtype=np.float64).reshape(H, W, 3)
    t = np.asarray(target, dtype=np.float64).reshape(H, W, 3)
    mp, mt = _filter_valid(p), _filter_valid(t)
    sp2 = _filter_valid(p * p) - mp * mp
    st2 = _filter_valid(t * t) - mt * mt
    spt = _filter_valid(p * t) - mp * mt
    s = ((2 * mp * mt + C1) * (2 * spt + C2)) / ((mp * mp + mt * mt + C1) * (sp2 + st2 + C2))
    return float(s.mean())


def ssim32_torchmetrics_form(pred, target, H, W):
    """fp32 throughout, as torchmetrics evaluates it on fp32 inputs."""
    import torch
    import torch.nn.functional as F
    pad = (WINDOW - 1) // 2
    p = torch.as_tensor(np.asarray(pred), dtype=torch.float32).reshape(1, H, W, 3).permute(0, 3, 1, 2)
    t = torch.as_tensor(np.asarray(target), dtype=torch.float32).reshape(1, H, W, 3).permute(0, 3, 1, 2)
    g = torch.as_tensor(weights()).float()
    kernel = (g[:, None] * g[None, :]).expand(3, 1, WINDOW, WINDOW).contiguous()
    p = F.pad(p, (pad, pad, pad, pad), mode="reflect")
    t = F.pad(t, (pad, pad, pad, pad), mode="reflect")
    stack = torch.cat([p, t, p * p, t * t, p * t])
    mp, mt, pp, tt, pt = F.conv2d(stack, kernel, groups=3).split(1)
    sp2, st2, spt = pp - mp * mp, tt - mt * mt, pt - mp * mt
    s = ((2 * mp * mt + C1) * (2 * spt + C2)) / ((mp * mp + mt * mt + C1) * (sp2 + st2 + C2))
    return float(s[..., pad:-pad, pad:-pad].mean())


# ---------------------------------------------------------------------------- seeded images
KINDS = ("noise", "smooth", "flat")


def image_pair(kind, H, W, seed):
    """(pred, target), each (H*W, 3) float32 in [0, 1]: uniform noise; a smooth sin image plus 0.02
    noise; a flat 0.9 image with 1e-3 noise (the near-flat bright window, where fp32 cancels)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        p, t = rng.random((H, W, 3)), rng.random((H, W, 3))
    elif kind == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        base = 0.5 + 0.4 * np.sin(0.11 * x[..., None] + 0.07 * y[..., None] + np.arange(3))
        p = base + 0.02 * (rng.random((H, W, 3)) - 0.5)
        t = base + 0.02 * (rng.random((H, W, 3)) - 0.5)
    elif kind == "flat":
        p = 0.9 + 1e-3 * (rng.random((H, W, 3)) - 0.5)
        t = 0.9 + 1e-3 * (rng.random((H, W, 3)) - 0.5)
    else:
        raise ValueError(kind)
    as32 = lambda a: np.clip(a, 0.0, 1.0).astype(np.float32).reshape(H * W, 3)  # noqa: E731
    return as32(p), as32(t)
