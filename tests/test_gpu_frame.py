"""The viewer frame path on the GPU (csrc/frame.hip, mfnerf.viewer): mfnerf_camera_rays and
mfnerf_frame_finish against the numpy restatements of tests/frame_ref.py at the kernels' seams,
FrameRenderer's captured graph against render_fused + the restated finish, and
Trainer.validate(save_dir=...)'s files against the device frames."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import frame_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
# frame.hip launches at most 2048 workgroups of 256 lanes: one pass covers 524288 output floats of
# camera_rays and as many 4-byte words of a frame (699050 pixels and a third)
PAST_ONE_PASS_WH = (800, 300)  # 720000 output floats per array
PAST_ONE_PASS_N = 700001


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ------------------------------------------------------------------------------------ camera_rays
def _camera(W, H, seed):
    """Off-centre principal point, fx != fy, a random rotation and origin."""
    g = np.random.default_rng(seed)
    q, r = np.linalg.qr(g.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    K = np.array([[37.3 + 0.11 * W, 0, 0.37 * W + 0.3], [0, 41.9 + 0.07 * H, 0.61 * H - 0.2], [0, 0, 1]], F32)
    pose = np.concatenate([q, g.normal(size=(3, 1))], 1).astype(F32)
    return K, pose


@pytest.mark.parametrize("W,H", [(1, 1), (63, 1), (65, 3), (257, 5), (64, 64), PAST_ONE_PASS_WH])
def test_camera_rays_sizes(gpu, W, H):
    from mfnerf import viewer
    K, pose = _camera(W, H, seed=W + H)
    o, d = viewer.camera_rays(K, _dev(pose, gpu), (W, H))
    assert o.shape == d.shape == (W * H, 3) and o.dtype == d.dtype == torch.float32
    o, d = o.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(_bits(o), _bits(np.broadcast_to(pose[:, 3], o.shape)))  # bit for bit
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    _, ref = frame_ref.camera_rays(K4, pose, W, H)
    err, bound = np.abs(d.astype(np.float64) - ref), frame_ref.camera_rays_bound(K4, pose, W, H)
    print(f"camera_rays {W}x{H}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_camera_rays_agree_with_the_torch_composition(gpu):
    """The route it replaces (data.get_ray_directions + get_rays) lands inside the same bound."""
    from mfnerf import data, viewer
    W, H = 65, 33
    K, pose = _camera(W, H, seed=5)
    o, d = viewer.camera_rays(K, _dev(pose, gpu), (W, H))
    to, td = data.get_rays(data.get_ray_directions(H, W, torch.from_numpy(K), device=gpu), _dev(pose, gpu))
    assert torch.equal(o, to.contiguous())
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    bound = frame_ref.camera_rays_bound(K4, pose, W, H)
    assert (np.abs(d.cpu().numpy().astype(np.float64) - td.cpu().numpy().astype(np.float64)) <= 2 * bound).all()


# ------------------------------------------------------------------------------------ frame_finish
def _finish(gpu, opacity, depth, rgb, mode, bg=0.0, workspace=None):
    """viewer.frame_finish on host arrays -> (frame_u8, frame_f32) as numpy."""
    from mfnerf import viewer
    t = [None if a is None else _dev(np.asarray(a, F32), gpu) for a in (opacity, depth, rgb)]
    u8, f32 = viewer.frame_finish(*t, mode=mode, bg=bg, workspace=workspace, want_f32=True)
    return u8.cpu().numpy(), f32.cpu().numpy()


def _colour_inputs(n):
    """rgb values exactly at k/255 and one ulp on either side, opacity 0 and 1 (and between), a blend
    one ulp above 1, blends far outside [0, 1], a NaN."""
    g = np.random.default_rng(n)
    k = (np.arange(256, dtype=F32) / F32(255)).astype(F32)
    special = np.stack([k, np.nextafter(k, F32(2)), np.nextafter(k, F32(-1))], 1).reshape(-1)  # 768 values
    rgb = g.uniform(-0.1, 1.1, 3 * n).astype(F32)
    m = min(3 * n, special.size)
    rgb[:m] = special[:m]
    rgb = rgb.reshape(n, 3)
    opacity = g.uniform(0, 1, n).astype(F32)
    opacity[0::4] = 1.0  # these rows keep rgb's exact values under either background
    opacity[1::4] = 0.0
    opacity[2::4] = 1.0
    if n > 2:
        rgb[n - 1] = (np.nextafter(F32(1), F32(2)), 1.0, 0.7)  # opaque: one ulp above 1, exactly 1
        opacity[n - 1] = 1.0
        rgb[n // 2, 1] = np.nan
    return opacity, rgb


@pytest.mark.parametrize("bg", [0.0, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, PAST_ONE_PASS_N])
def test_frame_finish_colour(gpu, n, bg):
    opacity, rgb = _colour_inputs(n)
    c = frame_ref.blend(opacity, rgb, bg)
    want = frame_ref.colour_u8(c)
    if n >= 257:  # the inputs reach what they are meant to
        assert (bg == 1.0 or len(np.unique(want)) == 256) and np.isnan(c).sum() == 1
        assert (c == np.nextafter(F32(1), F32(2))).any() and (c[~np.isnan(c)] * F32(255) < 0).any()
        assert bg == 0.0 or (c[~np.isnan(c)] * F32(255) >= 256).any()
    u8, f32 = _finish(gpu, opacity, None, rgb, "rgb", bg)
    assert u8.shape == (n, 3) and u8.dtype == np.uint8
    assert np.array_equal(u8, want)
    nan = np.isnan(c)
    assert np.array_equal(np.isnan(f32), nan) and np.array_equal(_bits(f32)[~nan], _bits(c)[~nan])


def _depth_cases():
    g = np.random.default_rng(7)
    n = 4099  # 17 workgroups of the range pass
    base = g.uniform(2, 6, n).astype(F32)
    lo_first = base.copy(); lo_first[0], lo_first[-1] = 1.0, 7.0
    hi_first = base.copy(); hi_first[0], hi_first[-1] = 7.0, 1.0
    every_k = (np.arange(2048, dtype=F32) * F32(0.37) + F32(3)).astype(F32)
    missed = base.copy(); missed[g.permutation(n)[: n // 2]] = 0.0
    big = g.uniform(2, 6, PAST_ONE_PASS_N).astype(F32)  # all 256 partial ranges, strided workgroups
    big[g.permutation(big.size)[: big.size // 2]] = 0.0
    big[-1] = 9.0
    return {"min_first_max_last": lo_first, "max_first_min_last": hi_first, "constant": np.full(n, 3.25, F32),
            "every_k": every_k, "half_missed": missed, "one_pixel": np.array([2.5], F32),
            "past_one_pass": big, "n65": base[:65].copy()}


_DEPTH = _depth_cases()


@pytest.mark.parametrize("case", list(_DEPTH))
def test_frame_finish_depth(gpu, case):
    from mfnerf import viewer
    depth = _DEPTH[case]
    want = frame_ref.depth2img(depth)
    if case == "every_k":
        x = (depth - depth.min()) / (depth.max() - depth.min())
        assert len(np.unique((x * F32(255)).astype(np.uint8))) == 256  # every k is produced
    if case == "constant":
        assert (want == frame_ref.lut()[0]).all()
    u8, f32 = _finish(gpu, None, depth, None, "depth")
    assert np.array_equal(u8, want)
    assert np.array_equal(_bits(f32), _bits(frame_ref.depth_f32(want)))
    # the same bits again, and with garbage in the workspace on entry (NaN patterns, then noise)
    ws = viewer.finish_workspace(gpu)
    for fill in (0xFF, None):
        if fill is None:
            ws.copy_(torch.randint(0, 256, ws.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(1)))
        else:
            ws.fill_(fill)
        again, again_f = _finish(gpu, None, depth, None, "depth", workspace=ws)
        assert np.array_equal(again, u8) and np.array_equal(_bits(again_f), _bits(f32))


# ------------------------------------------------------------------------------------ pipeline
class HP:
    pass


_model = {}


def _fixture_model(gpu):
    """The golden_render hash-rgb64 fixture's model (test_gpu_golden.py's `setup`)."""
    if "m" not in _model:
        from mfnerf.networks import NGP
        z = np.load(os.path.join(GOLD, "golden_render.npz"))
        meta = json.load(open(os.path.join(GOLD, "golden_render.json")))
        hp = HP()
        for k, v in meta["hparams"].items():
            setattr(hp, k, v)
        model = NGP(scale=meta["scale"], hparams=hp).to(gpu)
        with torch.no_grad():
            model.xyz_encoder.params.copy_(torch.from_numpy(z["xyz_params"]))
            model.rgb_net.params.copy_(torch.from_numpy(z["rgb_params"]))
            model.density_bitfield.copy_(torch.from_numpy(z["bitfield"]))
        _model["m"] = model
    return _model["m"]


W64 = 64
K64 = np.array([[0.5 * W64 / math.tan(0.5 * 0.6911112), 0, 32], [0, 0.5 * W64 / math.tan(0.5 * 0.6911112), 32],
                [0, 0, 1]], F32)


def _reference_frames(model, pose, gpu):
    """finish (the numpy restatement) of render_fused on the pose's rays, the rays from a call of
    camera_rays of their own: colour u8, colour f32, depth u8, depth f32, the render's results."""
    from mfnerf import rendering, viewer
    o, d = viewer.camera_rays(K64, pose.to(gpu).contiguous(), (W64, W64))
    res = rendering.render_fused(model, o, d, T_threshold=1e-2, max_samples=100)
    rgb, depth = res["rgb"].cpu().numpy(), res["depth"].cpu().numpy()
    du8 = frame_ref.depth2img(depth)
    shape = (W64, W64, 3)
    return {"rgb": frame_ref.colour_u8(rgb).reshape(shape), "rgb_f32": rgb.reshape(shape),
            "depth": du8.reshape(shape), "depth_f32": frame_ref.depth_f32(du8).reshape(shape), "res": res, "d": d}


def _frame(r, pose, mode, **kw):
    u8 = r.render(pose, mode, **kw)
    assert u8.shape == (W64, W64, 3) and u8.dtype == torch.uint8 and u8.is_cuda
    return u8.cpu().numpy(), r.frame_f32.cpu().numpy()


def test_pipeline(gpu):
    from mfnerf import synthetic, viewer
    model = _fixture_model(gpu)
    poses = synthetic.camera_poses()[:2]
    ref = [_reference_frames(model, p, gpu) for p in poses]
    hit = ref[0]["res"]["opacity"] > 0
    print("pipeline: rays with opacity > 0:", int(hit.sum()), "of", W64 * W64)
    assert int(hit.sum()) > 100  # the view holds the object
    assert not np.array_equal(ref[0]["rgb"], ref[1]["rgb"]) and not np.array_equal(ref[0]["depth"], ref[1]["depth"])
    r = viewer.FrameRenderer(model, K64, (W64, W64))
    assert (r.T_threshold, r.max_samples, r.exp_step_factor, r.bg) == (1e-2, 100, 0.0, 1.0)
    for mode in ("rgb", "depth"):
        # pose 0, pose 1 (the graph reads the pose buffer, not a baked pose), pose 0 again; poses
        # given as a tensor, a (4, 4) numpy matrix and a (3, 4) one
        p1 = np.concatenate([poses[1].numpy().astype(np.float64), [[0, 0, 0, 1]]])
        for i, pose in ((0, poses[0]), (1, p1), (0, poses[0].numpy())):
            u8, f32 = _frame(r, pose, mode)
            assert np.array_equal(u8, ref[i][mode]), (mode, i)
            assert np.array_equal(_bits(f32), _bits(ref[i][mode + "_f32"])), (mode, i)
            assert torch.equal(r.rays()[1], ref[i]["d"])
            assert torch.equal(r.rays()[0], poses[i][:, 3].to(gpu).expand(W64 * W64, 3))
            res = r.results()
            for k in ("opacity", "depth", "samples"):
                assert torch.equal(res[k], ref[i]["res"][k]), k
            assert int(res["total_samples"]) == int(ref[i]["res"]["total_samples"])
            # results()["rgb"] is the sum before the blend (bg = 1)
            blended = frame_ref.blend(res["opacity"].cpu().numpy(), res["rgb"].cpu().numpy(), 1.0)
            assert np.array_equal(_bits(blended.reshape(W64, W64, 3)), _bits(ref[i]["rgb_f32"]))
            assert torch.equal(r.mean_samples(), res["samples"].sum() / (W64 * W64))
            assert r.mean_samples().dim() == 0 and r.mean_samples().is_cuda
        eager_u8, eager_f32 = _frame(r, poses[1], mode, eager=True)
        assert np.array_equal(eager_u8, ref[1][mode]) and np.array_equal(_bits(eager_f32), _bits(ref[1][mode + "_f32"]))
    # to_host: a pinned copy and an event
    host, ev = r.to_host(r.render(poses[0], "rgb"))
    ev.synchronize()
    assert host.is_pinned() and np.array_equal(host.numpy(), ref[0]["rgb"])


def test_pipeline_follows_parameter_updates(gpu):
    """After an in-place update of the parameters the next frame (graph and eager) uses the new weights."""
    from mfnerf import synthetic, viewer
    model = _fixture_model(gpu)
    pose = synthetic.camera_poses()[0]
    r = viewer.FrameRenderer(model, K64, (W64, W64))
    before, _ = _frame(r, pose, "rgb")
    saved = model.rgb_net.params.detach().clone()
    try:
        with torch.no_grad():
            model.rgb_net.params.mul_(-0.5)
        want = _reference_frames(model, pose, gpu)
        after, _ = _frame(r, pose, "rgb")
        assert np.array_equal(after, want["rgb"]) and not np.array_equal(after, before)
        depth, _ = _frame(r, pose, "depth")
        assert np.array_equal(depth, want["depth"])
    finally:
        with torch.no_grad():
            model.rgb_net.params.copy_(saved)
    again, _ = _frame(r, pose, "rgb")
    assert np.array_equal(again, before)


# ------------------------------------------------------------------------------------ validate
@pytest.fixture(scope="module")
def trained(gpu):
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


@pytest.mark.parametrize("fused", [False, True], ids=["loop", "fused"])
def test_validate_writes_the_frames(gpu, trained, tmp_path, fused):
    from PIL import Image
    from mfnerf import data, rendering, viewer
    tr, imgs, poses, dirs, W = trained
    plain = tr.validate(imgs[:2], poses[:2], dirs, fused=fused)
    saved = tr.validate(imgs[:2], poses[:2], dirs, fused=fused, save_dir=str(tmp_path / "val"))
    assert saved == plain
    assert sorted(os.listdir(tmp_path / "val")) == ["000.png", "000_d.png", "001.png", "001_d.png"]
    model = tr.to_ngp()
    for i in range(2):
        o, d = data.get_rays(dirs.to(gpu), poses[i].to(gpu))
        res = rendering.render_fused(model, o, d) if fused else rendering.render(model, o, d, test_time=True)
        rgb, depth = res["rgb"].float().contiguous(), res["depth"].float().contiguous()
        colour, _ = viewer.frame_finish(res["opacity"].float().contiguous(), None, rgb, "rgb", 0.0)
        dimg, _ = viewer.frame_finish(None, depth, None, "depth")
        for name, frame, want in ((f"{i:03d}.png", colour, frame_ref.colour_u8(rgb.cpu().numpy())),
                                  (f"{i:03d}_d.png", dimg, frame_ref.depth2img(depth.cpu().numpy()))):
            im = Image.open(tmp_path / "val" / name)
            assert im.mode == "RGB" and im.size == (W, W)
            got = np.asarray(im)
            assert np.array_equal(got, frame.cpu().numpy().reshape(W, W, 3)), name
            assert np.array_equal(got, want.reshape(W, W, 3)), name
        assert len(np.unique(colour.cpu().numpy())) > 16 and len(np.unique(dimg.cpu().numpy(), axis=0)) > 16


@pytest.mark.parametrize("fused", [False, True], ids=["loop", "fused"])
def test_validate_writes_frames_of_an_odd_pixel_count(gpu, trained, tmp_path, fused):
    """33 x 31: 3 * W * H is no multiple of 4, so the two frames cannot share one allocation (each
    must start 4-byte aligned) and each frame's last word is a partial one."""
    from PIL import Image
    from mfnerf import data, rendering
    tr = trained[0]
    W, H = 33, 31
    poses = trained[2][:2]
    K = torch.tensor([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]])
    dirs = data.get_ray_directions(H, W, K)
    imgs = torch.rand(2, W * H, 3, generator=torch.Generator().manual_seed(3))
    plain = tr.validate(imgs, poses, dirs, img_wh=(W, H), fused=fused)
    saved = tr.validate(imgs, poses, dirs, img_wh=(W, H), fused=fused, save_dir=str(tmp_path / "odd"))
    assert saved == plain
    model = tr.to_ngp()
    for i in range(2):
        o, d = data.get_rays(dirs.to(gpu), poses[i].to(gpu))
        res = rendering.render_fused(model, o, d) if fused else rendering.render(model, o, d, test_time=True)
        for name, want in ((f"{i:03d}.png", frame_ref.colour_u8(res["rgb"].float().cpu().numpy())),
                           (f"{i:03d}_d.png", frame_ref.depth2img(res["depth"].float().cpu().numpy()))):
            im = Image.open(tmp_path / "odd" / name)
            assert im.size == (W, H)
            assert np.array_equal(np.asarray(im), want.reshape(H, W, 3)), name


# ------------------------------------------------------------------------------------ errors
def test_errors(gpu):
    from mfnerf import viewer
    from mfnerf._lib import call, ptr, stream
    from mfnerf.networks import NGP
    model = _fixture_model(gpu)
    n = 16
    k4 = (ctypes.c_float * 4)(50.0, 50.0, 2.0, 2.0)
    pose = torch.zeros(12, device=gpu)
    o, d = torch.empty(n, 3, device=gpu), torch.empty(n, 3, device=gpu)
    op, dep, rgb = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, 3, device=gpu)
    u8 = torch.empty(n, 3, dtype=torch.uint8, device=gpu)
    ws = viewer.finish_workspace(gpu)

    def rays(**over):
        a = dict(k4=k4, pose=ptr(pose), W=4, H=4, o=ptr(o), d=ptr(d))
        a.update(over)
        call("mfnerf_camera_rays", a["k4"], a["pose"], a["W"], a["H"], a["o"], a["d"], stream())

    def finish(**over):
        a = dict(op=ptr(op), dep=ptr(dep), rgb=ptr(rgb), n=n, mode=0, ws=ptr(ws), u8=ptr(u8))
        a.update(over)
        call("mfnerf_frame_finish", a["op"], a["dep"], a["rgb"], a["n"], a["mode"], 1.0, a["ws"], a["u8"], None,
             stream())

    for over in (dict(W=0), dict(H=0), dict(W=-1), dict(W=1 << 20, H=1 << 20)):
        with pytest.raises(RuntimeError, match="bad image size"):
            rays(**over)
    for name in ("k4", "pose", "o", "d"):
        with pytest.raises(RuntimeError, match="camera_rays: null pointer"):
            rays(**{name: None})
    with pytest.raises(RuntimeError, match="bad focal length"):
        rays(k4=(ctypes.c_float * 4)(0.0, 50.0, 2.0, 2.0))
    with pytest.raises(RuntimeError, match="unknown mode 2"):
        finish(mode=2)
    with pytest.raises(RuntimeError, match="bad n=-1"):
        finish(n=-1)
    for over in (dict(u8=None), dict(op=None), dict(rgb=None), dict(mode=1, dep=None), dict(mode=1, ws=None)):
        with pytest.raises(RuntimeError, match="frame_finish: null pointer"):
            finish(**over)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        finish(u8=ctypes.c_void_p(u8.data_ptr() + 1), n=n - 1)
    # what a mode does not read may be null; n = 0 is a no-op
    finish(dep=None, ws=None)
    finish(mode=1, op=None, rgb=None)
    finish(n=0, u8=None)
    rays()
    with pytest.raises(ValueError, match="unknown frame mode"):
        viewer.frame_finish(op, dep, rgb, mode="normals")
    with pytest.raises(RuntimeError, match="bad image size"):
        viewer.camera_rays(K64, pose, (0, 5))
    with pytest.raises(ValueError, match="img_wh must be positive"):
        viewer.FrameRenderer(model, K64, (0, 4))
    r = viewer.FrameRenderer(model, K64, (8, 8))
    with pytest.raises(ValueError, match="unknown frame mode"):
        r.render(np.eye(4), mode="normals")
    with pytest.raises(ValueError, match="pose must be"):
        r.render(np.eye(3))
    for bad in (torch.zeros(12, device=gpu), torch.zeros(3, 3, device=gpu)):  # device poses are checked alike
        with pytest.raises(ValueError, match="pose must be"):
            r.render(bad)
    r.render(torch.eye(4, device=gpu))

    class HDR:
        grid, L, F, T, N_min, N_max, N_tables, rgb_channels, rgb_layers = "Hash", 16, 2, 12, 4, 256, 1, 64, 2
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        viewer.FrameRenderer(NGP(0.5, HDR, rgb_act="None"), K64, (8, 8))
    torch.cuda.synchronize()
