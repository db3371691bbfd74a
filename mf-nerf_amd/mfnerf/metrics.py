"""The reference's validation metrics on the device (train.py:65-67, 198-237: torchmetrics
PeakSignalNoiseRatio(data_range=1) and StructuralSimilarityIndexMeasure(data_range=1), logged as
test/psnr and test/ssim).

    m = image_metrics(pred, target, (W, H))     # (2,) float64 on the device: [mse, ssim]
    psnr = psnr_from_mse(m[0])                  # still on the device

One HIP call (csrc/metrics.hip: mfnerf_image_metrics) computes both in fp64 from the fp32 images,
with no library convolution, no allocation when `out` and `workspace` are passed, and no host read:
a validation loop writes every view's pair into one tensor and reads it back once
(trainer.Trainer.validate), and the call can be captured in a graph.

SSIM is torchmetrics' value -- the 11x11 Gaussian window of sigma 1.5, c1 = 0.01^2, c2 = 0.03^2,
averaged over the pixels whose window lies inside the image, which is what remains after
torchmetrics pads by reflection and crops the padded border.  Parity with torchmetrics itself is
unpinned; tests/metrics_ref.py restates the definition twice.
"""
import torch

from ._lib import call, load, ptr, stream

# The kernel's output tile in pixels (csrc/metrics.hip MT_TH / MT_TW; a static_assert there names
# these two).  Shapes around a multiple of the tile plus the 10-pixel window border are the seams.
TILE_H = 16
TILE_W = 16
WINDOW = 11  # the Gaussian window; an image needs at least one whole window


def workspace_bytes(H, W):
    """Bytes of workspace image_metrics needs for an H x W image (one pair of doubles per tile)."""
    return int(load().mfnerf_image_metrics_workspace(int(H), int(W)))


def _check(name, t, rows):
    # argument errors come before the device check: a bad dtype or shape reads the same on any host
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be {torch.float32}, got {t.dtype}")
    if tuple(t.shape) != (rows, 3):
        raise RuntimeError(f"{name} must have shape (H*W, 3) = ({rows}, 3), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def image_metrics(pred, target, img_wh, out=None, workspace=None):
    """[mse, ssim] of pred against target, both (H*W, 3) float32 CUDA tensors (row-major pixels, rgb
    interleaved), img_wh = (W, H) as the datasets carry it -> a (2,) float64 tensor on their device.

    out (2,) float64 and workspace (uint8, at least workspace_bytes(H, W)) are allocated when not
    given; with both given the call allocates nothing.  The workspace needs no initialisation.
    RuntimeError for host tensors, non-contiguous input, a dtype other than float32, a shape other
    than (H*W, 3), or H or W below 11."""
    W, H = int(img_wh[0]), int(img_wh[1])
    if H < WINDOW or W < WINDOW:
        raise RuntimeError(f"image_metrics: H and W must be at least {WINDOW} (the SSIM window), got {H} x {W}")
    _check("pred", pred, H * W)
    _check("target", target, H * W)
    for name, t in (("pred", pred), ("target", target)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    if target.device != pred.device:
        raise RuntimeError("pred and target must be on the same device")
    dev = pred.device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (2,)
          or not out.is_contiguous() or out.device != dev):
        raise RuntimeError("out must be a contiguous (2,) float64 tensor on the images' device")
    need = workspace_bytes(H, W)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or not workspace.is_contiguous() or workspace.device != dev
          or workspace.numel() * workspace.element_size() < need or workspace.data_ptr() % 8):
        raise RuntimeError(f"workspace must be a contiguous 8-byte aligned tensor of at least {need} bytes on the "
                           "images' device")
    call("mfnerf_image_metrics", ptr(pred), ptr(target), H, W, ptr(out), ptr(workspace), stream())
    return out


def psnr_from_mse(mse):
    """PeakSignalNoiseRatio(data_range=1): 10 log10(1 / mse), element-wise on a tensor; no host read."""
    return -10.0 * torch.log10(mse)
