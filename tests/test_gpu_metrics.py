"""mfnerf_image_metrics (csrc/metrics.hip) against the fp64 restatement in metrics_ref.py.

Tolerances, derived rather than measured:
  |ssim - ref64| <= 1e-8.  Each moment is a 121-term convex sum of values in [0, 1], absolute error
      below 2e-14; the worst amplification is 1/c1 = 1e4 on the luminance factor and 1/c2 ~ 1.1e3 on
      the structure factor: a few 1e-10 relative per pixel on each side, doubled for the reference's
      own rounding.  A wrong tap, halo or tile seam is >= 1e-4.
  |mse - ref64| <= 3 H W 2^-52 ref64: a fixed-order fp64 sum of 3 H W exactly representable
      differences, squared.
"""
import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-8


def _mse_tol(H, W, ref):
    return 3 * H * W * 2.0 ** -52 * ref


def _run(gpu, p, t, H, W, **kw):
    from mfnerf.metrics import image_metrics
    out = image_metrics(torch.from_numpy(p).to(gpu), torch.from_numpy(t).to(gpu), (W, H), **kw)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2,) and out.device.type == "cuda"
    return out


def _check_case(gpu, H, W, case):
    kind = R.KINDS[case % len(R.KINDS)]
    p, t = R.image_pair(kind, H, W, seed=1000 + case)
    mse, ssim = _run(gpu, p, t, H, W).tolist()
    ref_mse, ref_ssim = R.mse64(p, t), R.ssim64(p, t, H, W)
    d_ssim, d_mse = abs(ssim - ref_ssim), abs(mse - ref_mse)
    print(f"{kind:6s} {H}x{W}: ssim {ssim:.12f} (|d| {d_ssim:.2e})  mse {mse:.6e} (|d|/ref {d_mse / ref_mse:.2e})")
    assert d_ssim <= SSIM_TOL, (kind, H, W, ssim, ref_ssim)
    assert d_mse <= _mse_tol(H, W, ref_mse), (kind, H, W, mse, ref_mse)


def _tile():
    from mfnerf import metrics
    return metrics.TILE_H, metrics.TILE_W


@pytest.mark.parametrize("wide", [False, True])
def test_height_sweep_across_tile_seams(gpu, wide):
    """Every H from one window to past the second tile seam, at one column of windows and at a width
    just past the first seam; the image kind alternates per case."""
    TH, TW = _tile()
    W = TW + 13 if wide else 11
    for case, H in enumerate(range(11, 2 * TH + 13)):
        _check_case(gpu, H, W, case + (50 if wide else 0))


@pytest.mark.parametrize("tall", [False, True])
def test_width_sweep_across_tile_seams(gpu, tall):
    TH, TW = _tile()
    H = TH + 13 if tall else 11
    for case, W in enumerate(range(11, 2 * TW + 13)):
        _check_case(gpu, H, W, case + (150 if tall else 100))


@pytest.mark.parametrize("case,H,W", [(0, 11, 11), (1, 200, 150), (2, 131, 257), (3, 257, 131)])
def test_one_window_and_many_tiles(gpu, case, H, W):
    _check_case(gpu, H, W, 200 + case)


@pytest.mark.parametrize("H,W", [(43, 37), (131, 257)])
def test_identical_images_give_exactly_zero_and_one(gpu, H, W):
    from mfnerf.metrics import image_metrics
    for kind in R.KINDS:
        p = torch.from_numpy(R.image_pair(kind, H, W, seed=7)[0]).to(gpu)
        assert image_metrics(p, p, (W, H)).tolist() == [0.0, 1.0]


def test_placement_and_no_reliance_on_memory_contents(gpu):
    """out may be a row of a larger tensor; the workspace may hold anything; nothing past H*W rows of
    the images is read."""
    from mfnerf.metrics import image_metrics, workspace_bytes
    H, W = 43, 37
    p, t = R.image_pair("smooth", H, W, seed=11)
    plain = _run(gpu, p, t, H, W)
    # row 1 of a NaN table
    table = torch.full((3, 2), float("nan"), dtype=torch.float64, device=gpu)
    _run(gpu, p, t, H, W, out=table[1])
    assert torch.isnan(table[0]).all() and torch.isnan(table[2]).all()
    assert torch.isfinite(table[1]).all() and torch.equal(table[1], plain)
    # NaN workspace (all-ones bytes are a NaN double), larger than needed
    ws = torch.full((workspace_bytes(H, W) + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    assert torch.isnan(ws.view(torch.float64)).all()
    assert torch.equal(_run(gpu, p, t, H, W, workspace=ws), plain)
    # NaN tail behind both images
    bp = torch.full((H * W + 4 * W, 3), float("nan"), device=gpu)
    bt = torch.full((H * W + 4 * W, 3), float("nan"), device=gpu)
    bp[:H * W] = torch.from_numpy(p).to(gpu)
    bt[:H * W] = torch.from_numpy(t).to(gpu)
    assert torch.equal(image_metrics(bp[:H * W], bt[:H * W], (W, H)), plain)


def test_two_calls_are_bit_identical(gpu):
    H, W = 131, 257
    p, t = R.image_pair("noise", H, W, seed=21)
    a, b = _run(gpu, p, t, H, W), _run(gpu, p, t, H, W)
    assert torch.equal(a, b)


def test_capture_and_replay(gpu):
    """One captured call on static buffers replays bit-identically to the eager call on whatever is
    copied into them."""
    from mfnerf.metrics import image_metrics, workspace_bytes
    H, W = 75, 70
    pairs = [[torch.from_numpy(a).to(gpu) for a in R.image_pair(kind, H, W, seed=31 + i)]
             for i, kind in enumerate(("noise", "flat"))]
    eager = [image_metrics(p, t, (W, H)).clone() for p, t in pairs]
    sp, st = pairs[0][0].clone(), pairs[0][1].clone()
    out = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu)
    ws = torch.empty(workspace_bytes(H, W), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        image_metrics(sp, st, (W, H), out=out, workspace=ws)
    for (p, t), ref in list(zip(pairs[::-1], eager[::-1])):
        sp.copy_(p)
        st.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    assert not torch.equal(eager[0], eager[1])


@pytest.mark.parametrize("H,W", [(10, 40), (40, 10)])
def test_too_small_an_image_is_an_error(gpu, H, W):
    from mfnerf._lib import call, ptr, stream
    from mfnerf.metrics import image_metrics
    p = torch.rand(H * W, 3, device=gpu)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu)
    ws = torch.empty(1024, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="at least 11"):
        image_metrics(p, p, (W, H), out=out, workspace=ws)
    with pytest.raises(RuntimeError, match=r"mfnerf_image_metrics failed \(1\).*at least 11"):
        call("mfnerf_image_metrics", ptr(p), ptr(p), H, W, ptr(out), ptr(ws), stream())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.fixture(scope="module")
def trained(gpu):
    """The 32x32 ball scene of test_trainer_evaluate_fused_opt_in: same HParams, 40 steps."""
    import math
    from mfnerf import data
    from mfnerf.trainer import HParams, Trainer
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    scene = data.BallScene(n_balls=6, seed=1)
    imgs, poses, dirs, K = data.ball_scene_views(scene, 8, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    tr = Trainer(HParams(batch_size=1024, T=16, num_epochs=1, steps_per_epoch=40), ds, device=gpu)
    tr.fit(log_every=0)
    return tr, imgs, poses, dirs, W


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_validate(gpu, trained, fused):
    from mfnerf import data, rendering
    from mfnerf.metrics import image_metrics, psnr_from_mse
    tr, imgs, poses, dirs, W = trained
    val = tr.validate(imgs[:2], poses[:2], dirs, fused=fused)
    assert set(val) == {"psnr", "ssim", "psnr_per_view", "ssim_per_view"}
    assert len(val["psnr_per_view"]) == len(val["ssim_per_view"]) == 2
    model = tr.to_ngp()
    for i in range(2):
        o, d = data.get_rays(dirs.to(gpu), poses[i].to(gpu))
        res = rendering.render_fused(model, o, d) if fused else rendering.render(model, o, d, test_time=True)
        pred, gt = res["rgb"].float().contiguous(), imgs[i].to(gpu, torch.float32).contiguous()
        m = image_metrics(pred, gt, (W, W))
        # 10 log10(1 / mse): the same fp64 value up to log10's rounding
        assert abs(val["psnr_per_view"][i] - float(psnr_from_mse(m[0]))) <= 1e-12 * abs(val["psnr_per_view"][i])
        assert val["ssim_per_view"][i] == float(m[1])
        ref = R.ssim64(pred.cpu().numpy(), gt.cpu().numpy(), W, W)
        print(f"fused={fused} view {i}: psnr {val['psnr_per_view'][i]:.4f} ssim {val['ssim_per_view'][i]:.10f} "
              f"(|d| vs ref64 {abs(val['ssim_per_view'][i] - ref):.2e})")
        assert abs(val["ssim_per_view"][i] - ref) <= SSIM_TOL
    assert val["psnr"] == sum(val["psnr_per_view"]) / 2
    assert val["ssim"] == sum(val["ssim_per_view"]) / 2
    mean_psnr, per_view = tr.evaluate(imgs[:2], poses[:2], dirs, fused=fused)
    for a, b in zip(val["psnr_per_view"], per_view):
        assert abs(a - b) <= 1e-3  # fp64 mean against evaluate's fp32 mean
    assert abs(val["psnr"] - mean_psnr) <= 1e-3
    assert 0.0 < val["ssim"] <= 1.0
