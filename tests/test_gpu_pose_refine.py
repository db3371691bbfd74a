"""Pose refinement inside the fused step on the GPU: the per-image reduction (mfnerf_pose_grad), the
pose optimizer and composition (mfnerf_pose_step), the draw that returns its indices
(mfnerf_sample_rays_prep_idx), the engine's refine_poses option (eager and replayed) and the trainer's
optimize_ext end to end.  References: tests/pose_ref.py (fp64)."""
import math

import pytest
import torch

import pose_ref as P
from mfnerf import data, engine, synthetic
from mfnerf._lib import call, ptr, stream

pytestmark = pytest.mark.gpu

GRAD_BOUND = 2e-5  # |err| <= 2e-5 * sum_r |u_r||g_r| per image row (dT rows: sum_r |g_o_r|)
HW = 50


# ------------------------------------------------------------------------------------- kernels
def _pose_grad(gpu, g_o, g_d, img, pix, poses, dirs, dR, amp=None):
    n_img = poses.shape[0]
    out = torch.full((2, n_img, 3), float("nan"), device=gpu)
    dev = [t.to(gpu).contiguous() for t in (g_o, g_d, img, pix, poses, dirs, dR)]
    call("mfnerf_pose_grad", *(ptr(t) for t in dev), g_o.shape[0], n_img, dirs.shape[0], ptr(out[0]), ptr(out[1]),
         ptr(amp), stream())
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu()


def _with_length(n_img, length, seed):
    ax = torch.randn(n_img, 3, generator=torch.Generator().manual_seed(seed))
    return (ax / ax.norm(dim=1, keepdim=True) * length).float()


def _check_pose_grad(got, ref, what):
    gR, gT = got
    rR, rT, A_R, A_T = ref
    for g, r, A, nm in ((gR, rR, A_R, "dR"), (gT, rT, A_T, "dT")):
        err = (g.double() - r).abs().max(dim=1).values
        ratio = float((err / A.clamp_min(1e-300)).max())
        print(f"{what} grad_{nm}: max |got - ref| / sum|terms| = {ratio:.3e} (bound {GRAD_BOUND:.0e})")
        assert torch.isfinite(g).all()
        assert (err <= GRAD_BOUND * A).all(), (what, nm, ratio)
        assert bool((g[A == 0] == 0).all()), "a row without rays must be zero"


@pytest.mark.parametrize("n_img", [1, 3, 70])
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 1000])
def test_pose_grad_matches_fp64(gpu, n_rays, n_img):
    """Random indices (one image forced empty when there are several), then every ray in one image;
    n_rays < n_img occurs at (1, 3), (1|63|64|65, 70); |dR| = 0, 1e-6, 1e-3, 0.1 each.  Per image row
    |err| <= 2e-5 * sum_r |u_r||g_r| (fp64 sum): per-term fp32 rounding of an O(1) Jacobian is a few
    6e-8, and the fixed-order sum of up to ~128 terms per lane adds at most 8e-6; a wrong Jacobian
    misses by O(1) of that sum.  Two runs give the same bits."""
    g = torch.Generator().manual_seed(1000 * n_img + n_rays)
    poses = synthetic.camera_poses(n_cams=n_img, seed=3)[:, :3].float().contiguous()
    dirs = torch.randn(HW, 3, generator=g)
    g_o = torch.randn(n_rays, 3, generator=g) * 1e-3
    g_d = torch.randn(n_rays, 3, generator=g) * 1e-3
    pix = torch.randint(0, HW, (n_rays,), generator=g, dtype=torch.int32)
    rand = torch.randint(0, n_img, (n_rays,), generator=g, dtype=torch.int32)
    empty = n_img // 2
    if n_img > 1:
        rand[rand == empty] = (empty + 1) % n_img
    one = torch.full((n_rays,), n_img - 1, dtype=torch.int32)
    for case, img in (("random", rand), ("one image", one)):
        for k, length in enumerate((0.0, 1e-6, 1e-3, 0.1)):
            dR = _with_length(n_img, length, seed=k)
            args = (g_o, g_d, img, pix, poses, dirs, dR)
            ref = P.pose_grad(*args)
            got = _pose_grad(gpu, *args)
            _check_pose_grad(got, ref, f"n_rays={n_rays} n_img={n_img} {case} |dR|={length:g}")
            again = _pose_grad(gpu, *args)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
            if n_img > 1:
                assert float(ref[2][empty]) == 0 and bool((got[0][empty] == 0).all())
    if n_rays < n_img:
        assert int((P.pose_grad(g_o, g_d, rand, pix, poses, dirs, dR)[2] == 0).sum()) >= n_img - n_rays


def test_pose_grad_raises_the_nonfinite_flag(gpu):
    n, n_img = 65, 3
    g = torch.Generator().manual_seed(4)
    poses = synthetic.camera_poses(n_cams=n_img, seed=3)[:, :3].float().contiguous()
    dirs = torch.randn(HW, 3, generator=g)
    g_o, g_d = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    img = torch.randint(0, n_img, (n,), generator=g, dtype=torch.int32)
    pix = torch.randint(0, HW, (n,), generator=g, dtype=torch.int32)
    dR = _with_length(n_img, 1e-3, 0)
    amp = torch.zeros(8, dtype=torch.int32, device=gpu)
    _pose_grad(gpu, g_o, g_d, img, pix, poses, dirs, dR, amp=amp)
    assert int(amp[0]) == 0
    bad = g_d.clone()
    bad[7, 1] = float("inf")
    gR, _ = _pose_grad(gpu, g_o, bad, img, pix, poses, dirs, dR, amp=amp)
    assert int(amp[0]) == 1 and not bool(torch.isfinite(gR[int(img[7])]).all())
    assert amp[1:].abs().sum().item() == 0
    _pose_grad(gpu, g_o, g_d, img, pix, poses, dirs, dR, amp=amp)  # a clean call never clears it
    assert int(amp[0]) == 1
    bad_o = g_o.clone()
    bad_o[3, 0] = float("nan")
    amp.zero_()
    _pose_grad(gpu, bad_o, g_d, img, pix, poses, dirs, dR, amp=amp)
    assert int(amp[0]) == 1


class _PoseState:
    def __init__(self, gpu, n_img, seed, zero=False):
        g = torch.Generator().manual_seed(seed)
        self.n = n_img
        self.poses = synthetic.camera_poses(n_cams=n_img, seed=seed)[:, :3].float().contiguous().to(gpu)
        dR = _with_length(n_img, 0.1, seed) * torch.rand(n_img, 1, generator=g)  # |dR| <= 0.1
        dR[::7] = 0.0
        dT = torch.randn(n_img, 3, generator=g) * 0.05
        if zero:
            dR, dT = torch.zeros_like(dR), torch.zeros_like(dT)
        self.dR, self.dT = dR.to(gpu), dT.to(gpu)
        self.m = torch.zeros(2, n_img, 3, device=gpu)
        self.v = torch.zeros(2, n_img, 3, device=gpu)
        self.step = torch.zeros(1, dtype=torch.int32, device=gpu)
        self.out = torch.full((n_img, 3, 4), float("nan"), device=gpu)

    def run(self, grads, lr, amp=None, lr_dev=None):
        gR, gT = (None, None) if grads is None else (grads[0], grads[1])
        call("mfnerf_pose_step", ptr(self.dR), ptr(self.dT), ptr(self.m), ptr(self.v), ptr(gR), ptr(gT),
             ptr(self.poses), self.n, lr, 0.9, 0.999, 1e-8, ptr(self.step), ptr(lr_dev), ptr(amp), ptr(self.out),
             stream())
        torch.cuda.synchronize()

    def snapshot(self):
        return [t.clone() for t in (self.dR, self.dT, self.m, self.v, self.step)]


def test_pose_step_matches_fp64_adam_and_composition(gpu):
    """Five steps on 300 images (more than the kernel's 256 threads) against fp64 Adam with the betas,
    eps and lr the ABI carries (fp32 values, widened): v within 1e-6 relative; m within 1e-6 of its sum
    of absolute terms (the same recurrence on |g|) and the offsets within 1e-6 of |p0| + sum |updates|
    -- relative to what was added, as a signed sum can cancel.  Rows 0..9 never see a gradient and stay
    put exactly; row 10 sees none from step 3 on, and its moments still move it.  poses_out within 1e-6
    absolute of the fp64 composition of the fp64 offsets (|dR| <= 0.1 + 5e-3)."""
    n_img, lr = 300, 1e-3
    s = _PoseState(gpu, n_img, seed=2)
    p0 = torch.stack([s.dR.cpu(), s.dT.cpu()])
    ref = P.Adam64(p0, lr)
    g = torch.Generator().manual_seed(9)
    lr_dev = torch.full((1,), lr, device=gpu)
    for k in range(5):
        grads = torch.randn(2, n_img, 3, generator=g) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
        grads[:, :10] = 0.0
        if k >= 3:
            grads[:, 10] = 0.0
        before = s.dR[10].clone()
        s.run(grads.to(gpu), 123.0, lr_dev=lr_dev)  # the device learning rate wins
        ref.step(grads)
        assert int(s.step) == k + 1
        if k >= 3:
            assert not torch.equal(s.dR[10], before), "a zero-gradient row still moves on its moments"
    got_p = torch.stack([s.dR.cpu(), s.dT.cpu()]).double()
    e_v = float(((s.v.cpu().double() - ref.v).abs() / ref.v.clamp_min(1e-300)).max())
    e_m = float(((s.m.cpu().double() - ref.m).abs() / ref.m_abs.clamp_min(1e-300)).max())
    e_p = float(((got_p - ref.p).abs() / (p0.double().abs() + ref.moved).clamp_min(1e-300)).max())
    want = P.compose(s.poses.cpu(), ref.p[0], ref.p[1])
    e_c = float((s.out.cpu().double() - want).abs().max())
    print(f"pose_step after 5 steps: v {e_v:.3e}, m {e_m:.3e}, offsets {e_p:.3e} (relative), poses_out {e_c:.3e} (absolute)")
    assert e_v <= 1e-6 and e_m <= 1e-6 and e_p <= 1e-6
    assert e_c <= 1e-6
    assert torch.equal(got_p[:, :10].float(), p0[:, :10]) and float(s.m[:, :10].abs().max()) == 0
    assert float(ref.moved[:, 11:].min()) > 0


def test_pose_step_zero_offsets_reproduce_the_base_poses(gpu):
    for n_img in (1, 70, 300):
        s = _PoseState(gpu, n_img, seed=5, zero=True)
        s.run(None, 0.0)                                   # the composition alone
        assert torch.equal(s.out, s.poses) and int(s.step) == 0
        s.out.fill_(float("nan"))
        s.run(torch.randn(2, n_img, 3).to(gpu), 0.0)       # an update at lr 0 leaves the offsets zero
        assert torch.equal(s.out, s.poses) and int(s.step) == 1
        assert float(s.dR.abs().max()) == 0 and float(s.dT.abs().max()) == 0


def test_pose_step_skips_on_the_nonfinite_flag(gpu):
    n_img = 70
    s = _PoseState(gpu, n_img, seed=6)
    grads = torch.randn(2, n_img, 3, generator=torch.Generator().manual_seed(1)).to(gpu)
    s.run(grads, 1e-3)
    snap = s.snapshot()
    s.run(None, 0.0)
    composed = s.out.clone()
    amp = torch.zeros(8, dtype=torch.int32)
    amp[0], amp[1], amp[3], amp[4] = 1, 3, 17, 2000
    amp.view(torch.float32)[2] = 1234.0
    amp_dev = amp.to(gpu)
    s.out.fill_(float("nan"))
    s.run(grads, 1e-3, amp=amp_dev)
    for a, b in zip(snap, s.snapshot()):
        assert torch.equal(a, b)
    assert torch.equal(s.out, composed), "poses_out is still composed from the unchanged offsets"
    assert torch.equal(amp_dev.cpu(), amp), "nothing of the amp state is written (skipped, scale, ticket, flag)"
    amp_dev[0] = 0
    s.run(grads, 1e-3, amp=amp_dev)                        # flag down: the step is taken
    assert int(s.step) == 2 and not torch.equal(s.dT, snap[1])
    assert torch.equal(amp_dev.cpu()[1:], amp[1:])


def _tiny_dataset(gpu, seed=5, n_img=5):
    g = torch.Generator().manual_seed(11)
    images = torch.rand(n_img, HW, 3, generator=g)
    poses = synthetic.camera_poses(n_cams=n_img, seed=1)[:, :3].float()
    dirs = torch.randn(HW, 3, generator=g)
    return data.DeviceDataset(images, poses, dirs, device=gpu, seed=seed)


@pytest.mark.parametrize("strategy", ["all_images", "same_image"])
def test_sample_rays_prep_idx_is_the_prep_draw_plus_indices(gpu, strategy):
    """Two calls (call counter 0 and 1) of three datasets with one seed: prep + indices gives the bits
    of prep, and the indices of the plain draw; poses= replaces the poses the rays are formed from."""
    n = 321
    a, b, c = (_tiny_dataset(gpu) for _ in range(3))
    for d in (a, b, c):
        d.same_image = {"all_images": 0, "same_image": 1}[strategy]
    center, half = torch.zeros(1, 3, device=gpu), torch.full((1, 3), 0.5, device=gpu)

    def bufs():
        return (torch.zeros(3, n, 3, device=gpu), torch.zeros(n, 1, 2, device=gpu), torch.zeros(n, device=gpu),
                torch.full((n,), -1, dtype=torch.int32, device=gpu), torch.full((n,), -1, dtype=torch.int32, device=gpu))

    for _ in range(2):
        oa, ha, na, ia, pa = bufs()
        ob, hb, nb, _, _ = bufs()
        oc, _, _, ic, pc = bufs()
        a.sample(oa, prep=(center, half, 0.01, ha, na), img_idx=ia, pix_idx=pa)
        b.sample(ob, prep=(center, half, 0.01, hb, nb))
        c.sample(oc, img_idx=ic, pix_idx=pc)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ha, hb) and torch.equal(na, nb)
        assert torch.equal(ia, ic) and torch.equal(pa, pc)
        assert int(ia.min()) >= 0 and int(ia.max()) < a.n_img and int(pa.min()) >= 0 and int(pa.max()) < HW
        assert torch.equal(oa[0], a.poses[ia.long(), :, 3])
        if strategy == "same_image":
            assert int(ia.min()) == int(ia.max())
    moved = a.poses.clone()
    moved[:, :, 3] += 0.25
    oa, ha, na, ia, pa = bufs()
    a.sample(oa, prep=(center, half, 0.01, ha, na), img_idx=ia, pix_idx=pa, poses=moved)
    torch.cuda.synchronize()
    assert torch.equal(oa[0], moved[ia.long(), :, 3])
    with pytest.raises(ValueError, match="poses="):
        a.sample(oa, prep=(center, half, 0.01, ha, na), poses=moved[:2])


# -------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def views(gpu):
    """12 analytic 16x16 views of the balls the occupancy prior marks (shared, never modified)."""
    W = 16
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    return data.ball_scene_views(data.BallScene.matching_grid(), 12, W, focal, seed=0, device=gpu)


def _engine(gpu, views, **kw):
    """_engine of test_gpu_input_grad.py (256 rays, log2_T = 14) with a device dataset attached."""
    imgs, poses, dirs, _ = views
    st = engine.TrainStep(engine.StepConfig(n_rays=256, log2_T=14, **kw), device=gpu, seed=0)
    st.set_occupancy(synthetic.ball_density_grid())
    st.attach_dataset(data.DeviceDataset(imgs, poses, dirs, device=gpu, seed=5))
    return st


def _field_state(st):
    return [t.clone() for t in (st.params, st.m, st.v, st.p16)]


def test_engine_refine_poses_at_lr_zero_is_the_ray_grads_step(gpu, views):
    """Three steps: refine_poses at pose_lr = 0 leaves the field's params, m, v and p16 bit-identical
    to a ray_grads step on the same dataset seed, dR / dT stay zero; captured and replayed it gives the
    eager bits."""
    a = _engine(gpu, views, refine_poses=True, pose_lr=0.0)
    b = _engine(gpu, views, ray_grads=True)
    c = _engine(gpu, views, refine_poses=True, pose_lr=0.0)
    for _ in range(3):
        a.run()
        b.run()
    torch.cuda.synchronize()
    assert not hasattr(b, "dR") and not hasattr(b.mbuf[0], "img_idx")
    for x, y in zip(_field_state(a), _field_state(b)):
        assert torch.equal(x, y)
    assert float(a.dR.abs().max()) == 0 and float(a.dT.abs().max()) == 0 and int(a.pose_step_dev) == 3
    assert float(a.pose_grad.abs().max()) > 0 and a.skipped_steps() == 0
    assert torch.equal(a.pose_buf[0], a.dataset.poses)
    c.run()
    torch.cuda.synchronize()
    c.capture()
    for _ in range(2):
        c.replay()
    torch.cuda.synchronize()
    for x, y in zip(_field_state(c), _field_state(a)):
        assert torch.equal(x, y)
    assert torch.equal(c.pose_grad, a.pose_grad) and torch.equal(c.pose_m, a.pose_m)
    assert float(c.dR.abs().max()) == 0 and float(c.dT.abs().max()) == 0
    assert c.gate_timeouts() == 0


def _ref_from_step(st, dR_before):
    t, mb, ds = st.parts[0], st.state.march, st.dataset
    return P.pose_grad(t.dL_drays_o.cpu(), t.dL_drays_d.cpu(), mb.img_idx.cpu(), mb.pix_idx.cpu(), ds.poses.cpu(),
                       ds.directions.cpu(), dR_before.cpu())


def test_engine_refine_poses_eager_step(gpu, views):
    """pose_lr > 0, eager: the step's grad_dR / grad_dT equal pose_ref on the step's own dL_drays_* and
    indices within the kernel bound, and dR / dT equal fp64 Adam on those gradients (offsets within 1e-6
    of sum |updates|) -- after the first step (dR = 0) and after the second (|dR| ~ 1e-3)."""
    lr = 1e-3
    st = _engine(gpu, views, refine_poses=True, pose_lr=lr)
    ref = P.Adam64(torch.zeros(2, st.dataset.n_img, 3), lr)
    for k in range(2):
        dR_before = st.dR.clone()
        st.run()
        torch.cuda.synchronize()
        assert st.skipped_steps() == 0
        got = (st.pose_grad[0].cpu(), st.pose_grad[1].cpu())
        _check_pose_grad(got, _ref_from_step(st, dR_before), f"engine step {k}")
        assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0
        ref.step(st.pose_grad.cpu())
        got_p = torch.stack([st.dR.cpu(), st.dT.cpu()]).double()
        e_p = float(((got_p - ref.p).abs() / ref.moved.clamp_min(1e-300)).max())
        print(f"engine step {k}: offsets vs fp64 Adam {e_p:.3e} (relative to sum |updates|)")
        assert e_p <= 1e-6
        # eager: no lag -- the buffer the next draw reads already holds this step's offsets
        assert torch.equal(st.pose_buf[0][:, :, 3], st.dataset.poses[:, :, 3] + st.dT)
    assert float(st.dR.abs().max()) > 0 and float(st.dT.abs().max()) > 0


def _replayed_run(gpu, views, steps=6):
    st = _engine(gpu, views, refine_poses=True, pose_lr=1e-3)
    st.run()
    torch.cuda.synchronize()
    st.capture()
    torch.cuda.synchronize()
    t0 = st.dataset.poses[:, :, 3]
    hist = {-1: st.dT.clone()}  # the offsets the capture composed both buffers from
    for k in range(steps):
        st.replay()
        torch.cuda.synchronize()
        hist[k] = st.dT.clone()
        seen = hist[max(k - 2, -1)]
        img = st.state.march.img_idx.long()
        assert torch.equal(st.last_batch.rays_o, (t0 + seen)[img]), f"step {k}: the draw did not read dT of step {k - 2}"
        if k >= 2:
            assert not torch.equal(hist[k - 1], hist[k - 2])
    assert st.gate_timeouts() == 0 and st.skipped_steps() == 0
    return st


def test_engine_refine_poses_replayed_lag_and_determinism(gpu, views):
    """Six replayed steps: step k's rays_o equal t0[img] + dT after step k-2, bit for bit (the
    documented one-step lag: the draw of step k runs beside step k-1 and reads the buffer step k-2
    wrote; steps 0 and 1 read what capture() composed).  Two identical runs give identical bits; no
    gated march ran on its timeout."""
    a = _replayed_run(gpu, views)
    b = _replayed_run(gpu, views)
    for x, y in zip(_field_state(a) + [a.dR, a.dT, a.pose_m, a.pose_v],
                    _field_state(b) + [b.dR, b.dT, b.pose_m, b.pose_v]):
        assert torch.equal(x, y)
    assert int(a.pose_step_dev) == 7 and float(a.dR.abs().max()) > 0


def test_engine_refine_poses_skips_with_the_field_on_a_nonfinite_step(gpu, views):
    """A loss scale far too large overflows the fp16 backward (as test_gpu_optim.py forces it): the
    pose state stays as it was and the skip count advances by one -- counted once, by the field's
    optimizer pass."""
    st = _engine(gpu, views, refine_poses=True, pose_lr=1e-3)
    for _ in range(2):
        st.run()
    torch.cuda.synchronize()
    assert st.skipped_steps() == 0
    snap = [t.clone() for t in (st.dR, st.dT, st.pose_m, st.pose_v, st.pose_step_dev, st.params)]
    st.reset_loss_scale(2.0 ** 40)
    st.run()
    torch.cuda.synchronize()
    assert st.skipped_steps() == 1 and st.loss_scale() == 2.0 ** 39
    for x, y in zip(snap, (st.dR, st.dT, st.pose_m, st.pose_v, st.pose_step_dev, st.params)):
        assert torch.equal(x, y)
    assert torch.equal(st.pose_buf[0][:, :, 3], st.dataset.poses[:, :, 3] + st.dT)


# ---------------------------------------------------------------------------------- end to end
# The parent's eager route under the same protocol (PoseRefiner.optimizer(1e-3) + render(), frozen
# field, 1024 random rays of all 40 images per step, E2E_STEPS steps) brings |dT[7] + offset| to
# RHO_EAGER of its start; measured once by tools/pose_refine_bench.py --e2e on an MI355X and recorded
# in profiles/r09_pose_refine.json ("e2e") with the fused route's ratio.
E2E_STEPS = 200
# Two runs gave 0.528 and 0.562 (the eager route's float atomics vary); the smaller, stricter one is
# taken.  The fused route measured 0.642 both times (it is bit-reproducible); the bound is 0.727.
RHO_EAGER = 0.528


def test_optimize_ext_recovers_a_translation_offset(gpu, tmp_path):
    """The 32x32 ball scene trained for 400 steps (as test_pose_gradient_points_along_a_translation_offset),
    checkpointed; image 7's translation moved by (0.03, -0.02, 0.025); a new Trainer(optimize_ext,
    pose_lr 1e-3) loads the checkpoint, freezes the field (set_lr(0)) and replays E2E_STEPS steps:
    |dT[7] + offset| falls to at most sqrt(RHO_EAGER) of its start -- half the eager route's
    log-reduction, the margin for the different batches and the one-step lag; a sign or Jacobian error
    gives a ratio of at least 1.  The checkpoint round-trips dR / dT."""
    from mfnerf.trainer import HParams, Trainer
    assert RHO_EAGER is not None and 0 < RHO_EAGER < 1
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    imgs, poses, dirs, K = data.ball_scene_views(data.BallScene(n_balls=6, seed=1), 40, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    hp = HParams(batch_size=1024, T=14, num_epochs=1, steps_per_epoch=400)
    tr = Trainer(hp, ds, device=gpu)
    tr.fit(log_every=0)
    ck = str(tmp_path / "field.ckpt")
    tr.save(ck)
    assert "dR" not in tr.state_dict()
    offset = torch.tensor([0.03, -0.02, 0.025])
    moved = poses.clone()
    moved[7, :3, 3] += offset
    ds2 = data.DeviceDataset(imgs, moved, dirs, K=K, img_wh=(W, W), device=gpu, seed=6)
    hp2 = HParams(batch_size=1024, T=14, num_epochs=1, steps_per_epoch=400, optimize_ext=True, pose_lr=1e-3)
    tr2 = Trainer(hp2, ds2, device=gpu)
    tr2.load(ck)
    tr2.step.set_lr(0.0)
    p0 = tr2.step.params.clone()
    for _ in range(E2E_STEPS + 1):  # the first call runs eagerly and captures
        tr2.training_step()
    torch.cuda.synchronize()
    assert torch.equal(tr2.step.params, p0), "the field is frozen"
    rho = float((tr2.step.dT[7].cpu() + offset).norm() / offset.norm())
    print(f"fused |dT[7] + offset| ratio after {E2E_STEPS} steps: {rho:.4f} "
          f"(eager route {RHO_EAGER:.4f}, bound sqrt = {math.sqrt(RHO_EAGER):.4f})")
    assert tr2.step.skipped_steps() == 0 and tr2.step.gate_timeouts() == 0
    assert rho <= math.sqrt(RHO_EAGER)
    # refined_poses() is the composition of the current offsets; the checkpoint carries dR / dT back
    want = P.compose(moved[:, :3], tr2.step.dR.cpu(), tr2.step.dT.cpu())
    assert float((tr2.refined_poses().cpu().double() - want).abs().max()) <= 1e-6
    ck2 = str(tmp_path / "posed.ckpt")
    tr2.save(ck2)
    sd = torch.load(ck2, map_location="cpu", weights_only=True)["state_dict"]
    assert torch.equal(sd["dR"], tr2.step.dR.cpu()) and torch.equal(sd["dT"], tr2.step.dT.cpu())
    assert torch.equal(sd["poses"], moved[:, :3].float())
    tr3 = Trainer(hp2, ds2, device=gpu)
    tr3.load(ck2)
    torch.cuda.synchronize()
    assert torch.equal(tr3.step.dR, tr2.step.dR) and torch.equal(tr3.step.dT, tr2.step.dT)
    assert float(tr3.step.pose_m.abs().max()) == 0 and int(tr3.step.pose_step_dev) == 0
    for buf in tr3.step.pose_buf:  # both buffers recomposed from the loaded offsets
        assert torch.equal(buf[:, :, 3], ds2.poses[:, :, 3] + tr3.step.dT)
