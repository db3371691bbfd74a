"""--random_bg inside the fused step on the GPU: the device-colour forms of the two loss-carrying
kernels against their scalar forms (bit for bit), the draw that writes the batch's colour
(mfnerf_sample_rays_prep_bg) against the NumPy definition tests/bg_ref.py, the engine's random_bg
option eagerly and replayed (the colour belongs to the batch), and the trainer end to end.

Bit-for-bit comparisons need no tolerance.  The one place where two launches of the SAME kernel may
differ is mfnerf_nerf_loss's loss_sum: each wave adds its partial sum with one float atomic, in arrival
order.  One wave (n_rays <= 64) has one order; more waves have several, so there the two forms' sums
are held to the reordering bound -- every one of the w = ceil(n_rays/64) additions rounds by at most
2^-24 of the running sum, which never exceeds start + loss, so two orders differ by at most
2 w 2^-24 (start + loss) -- while the gradients, which no atomic touches, stay bit for bit.
The fp64 checks of the eager step use the bounds tests/test_gpu_vren_seams.py derives for
mfnerf_nerf_loss: gradients within 16 * 2^-24 of their maximum, the loss within 64 * 2^-24 |loss| +
8 * 2^-24 (start + |loss|), start = 0 here.

Measured on an MI355X (every test prints its figures): the eager step's E(dL_drgb) <= 1.2e-7 and
E(dL_dopacity) <= 1.4e-7 against 9.5e-7 in all three variants, |loss - ref| <= 2.9e-8 against >= 6.9e-7;
the five-wave loss sums of the two forms differed by at most one ulp (6.0e-8 against a bound of 5.0e-7)."""
import functools
import math

import numpy as np
import pytest
import torch

import bg_ref as B
import composite_ref as R
from mfnerf import data, engine, synthetic
from mfnerf._lib import call, ptr, stream
from test_gpu_pose_refine import _field_state, _tiny_dataset
from test_gpu_vren_seams import EPS, LAMBDA, NAN, SENT, THR, _outs

pytestmark = pytest.mark.gpu

COLOURS = [(0.2, 0.5, 0.9), (0.0, 0.0, 0.0)]


def _bg_in_nan_buffer(gpu, colour):
    """The 3 floats at an odd 4-byte offset (word 3: byte 12) of a buffer whose other words hold NaN."""
    buf = torch.full((8,), NAN, device=gpu)
    buf[3:6] = torch.tensor(colour, device=gpu)
    return buf, buf[3:6]


# ------------------------------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def seam(gpu):
    b = R.seam_rays(0)
    g = R.seam_grads(b)
    s = dict(n_rays=b["rays_a"].shape[0], n=b["in_ray"].shape[0], target=g["target"].to(gpu))
    assert (s["n_rays"], s["n"]) == (93, 22373)
    s["dev"] = {k: b[k].to(gpu) for k in ("sigmas", "rgbs", "deltas", "ts", "rays_a")}
    return s


@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("mean_x", [1, 4])
def test_composite_fused_bg_equals_the_scalar_form(gpu, seam, mean_x, colour):
    s, d, n_rays, n = seam, seam["dev"], seam["n_rays"], seam["n"]
    n_mean = mean_x * n_rays
    buf, bg = _bg_in_nan_buffer(gpu, colour)
    assert bg.data_ptr() % 8 == 4
    head = (ptr(d["sigmas"]), ptr(d["rgbs"]), ptr(d["deltas"]), ptr(d["ts"]), ptr(d["rays_a"]), n_rays, n, THR,
            ptr(s["target"]), n_mean, LAMBDA)

    def tail(o):
        return (ptr(o["total"]), ptr(o["op"]), ptr(o["de"]), ptr(o["rgb"]), ptr(o["ws"]), ptr(o["g_rgb"]), ptr(o["g_op"]),
                ptr(o["dsig"]), ptr(o["drgb"]), ptr(o["loss"]), stream())

    a, c = _outs(s, gpu), _outs(s, gpu)
    call("mfnerf_composite_train_fused_bg", *head, ptr(bg), *tail(a))
    call("mfnerf_composite_train_fused", *head, *colour, *tail(c))
    torch.cuda.synchronize()
    for k in a:
        assert not torch.isnan(c[k]).any(), k     # every row written (so equal means equal bits' values)
        assert torch.equal(a[k], c[k]), k
        assert torch.equal(a[k].view(torch.int64 if k == "total" else torch.int32),
                           c[k].view(torch.int64 if k == "total" else torch.int32)), k
    # the colour matters (the comparison is not vacuous) and the buffer around it is as it was
    if any(colour):
        z = _outs(s, gpu)
        call("mfnerf_composite_train_fused", *head, 0.0, 0.0, 0.0, *tail(z))
        torch.cuda.synchronize()
        assert not torch.equal(z["g_rgb"], a["g_rgb"]) and torch.equal(z["rgb"], a["rgb"])
    assert torch.isnan(buf[:3]).all() and torch.isnan(buf[6:]).all()
    assert torch.equal(buf[3:6].cpu(), torch.tensor(colour))


@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 257])
def test_nerf_loss_bg_equals_the_scalar_form(gpu, n_rays, colour):
    g = torch.Generator().manual_seed(100 + n_rays)
    rgb, op = torch.rand(n_rays, 3, generator=g), torch.rand(n_rays, generator=g)
    gt = torch.rand(n_rays, 3, generator=g)
    op[-1] = 0.0
    if n_rays > 1:
        op[0] = 1.0
    n_mean, start, guard = 2 * n_rays, 0.75, 64
    RGB, OP, GT = rgb.to(gpu), op.to(gpu), gt.to(gpu)
    buf, bg = _bg_in_nan_buffer(gpu, colour)
    waves = -(-n_rays // 64)
    for with_sum in (True, False):
        res = []
        for form in ("_bg", ""):
            g_rgb = torch.full((n_rays + guard, 3), SENT, device=gpu)
            g_op = torch.full((n_rays + guard,), SENT, device=gpu)
            loss = torch.full((1,), start, device=gpu)
            bg_args = (ptr(bg),) if form else colour
            call("mfnerf_nerf_loss" + form, ptr(RGB), ptr(OP), ptr(GT), n_rays, n_mean, LAMBDA, *bg_args, ptr(g_rgb),
                 ptr(g_op), ptr(loss if with_sum else None), stream())
            torch.cuda.synchronize()
            assert (g_rgb[n_rays:] == SENT).all() and (g_op[n_rays:] == SENT).all(), "guard rows written"
            res.append((g_rgb.cpu(), g_op.cpu(), float(loss)))
        (c1, o1, l1), (c0, o0, l0) = res
        assert torch.equal(c1.view(torch.int32), c0.view(torch.int32))
        assert torch.equal(o1.view(torch.int32), o0.view(torch.int32))
        if not with_sum:
            assert l1 == start and l0 == start
        elif waves == 1:
            assert l1 == l0 and l1 != start
        else:
            bound = 2 * waves * EPS * max(l0, l1)
            print(f"nerf_loss_bg n={n_rays} ({waves} waves' atomics): |loss_bg - loss| = {abs(l1 - l0):.3e} "
                  f"(reordering bound {bound:.3e})")
            assert abs(l1 - l0) <= bound and l1 != start
    assert torch.isnan(buf[:3]).all() and torch.isnan(buf[6:]).all()


# ---------------------------------------------------------------------------------------- draw
@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("strategy", ["all_images", "same_image"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sample_rays_prep_bg_draws_the_reference_colour(gpu, n, strategy, with_idx):
    """Five calls in a row: call k's colour is bg_ref.bg_colour(seed, k) exactly -- whatever n_rays, the
    strategy or the index outputs -- every other output has the bits of the same call sequence on a
    twin dataset without bg, and the words around the 3 floats keep their sentinel."""
    seed = 5
    a, b = _tiny_dataset(gpu, seed=seed), _tiny_dataset(gpu, seed=seed)
    for d in (a, b):
        d.same_image = {"all_images": 0, "same_image": 1}[strategy]
    center, half = torch.zeros(1, 3, device=gpu), torch.full((1, 3), 0.5, device=gpu)

    def bufs():
        return (torch.full((3, n, 3), SENT, device=gpu), torch.full((n, 1, 2), SENT, device=gpu),
                torch.full((n,), SENT, device=gpu), torch.full((n,), -1, dtype=torch.int32, device=gpu),
                torch.full((n,), -1, dtype=torch.int32, device=gpu))

    seen = []
    for k in range(5):
        oa, ha, na, ia, pa = bufs()
        ob, hb, nb, ib, pb = bufs()
        buf = torch.full((9,), SENT, device=gpu)
        idx_a = dict(img_idx=ia, pix_idx=pa) if with_idx else {}
        idx_b = dict(img_idx=ib, pix_idx=pb) if with_idx else {}
        a.sample(oa, prep=(center, half, 0.01, ha, na), bg=buf[3:6], **idx_a)
        b.sample(ob, prep=(center, half, 0.01, hb, nb), **idx_b)
        torch.cuda.synchronize()
        want = B.bg_colour(seed, k)
        got = buf[3:6].cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, got, want)
        assert (buf[:3] == SENT).all() and (buf[6:] == SENT).all()
        for x, y in ((oa, ob), (ha, hb), (na, nb), (ia, ib), (pa, pb)):
            assert torch.equal(x, y)
        assert not (oa == SENT).any() and bool((ia >= 0).all()) == with_idx
        assert int(a.calls[0]) == k + 1 and int(a.calls[1]) == 0
        seen.append(tuple(got.tolist()))
    assert len(set(seen)) == 5
    with pytest.raises(ValueError, match="prep="):
        a.sample(oa, bg=buf[3:6])


# -------------------------------------------------------------------------------------- engine
@functools.lru_cache(maxsize=None)
def _real_grid():
    return synthetic.ball_density_grid(cascades=2, scale=1.0)


def _real_step(gpu, **kw):
    """256 rays, log2_T = 14 on a real-scene box (scale 1: two cascades, exponential steps, black
    background) around the ball-union occupancy."""
    st = engine.TrainStep(engine.StepConfig(n_rays=256, log2_T=14, scale=1.0, **kw), device=gpu, seed=0)
    assert st.cascades == 2
    st.set_occupancy(_real_grid())
    return st


def _given(gpu, st):
    batch = st.make_batches(1, seed=1)[0]
    noise = torch.rand(st.cfg.n_rays, generator=torch.Generator().manual_seed(3)).to(gpu)
    return batch, noise


def _check_parts_against_fp64(st, batch, what):
    """Every part's dL_drgb / dL_dopacity and the step's NeRF loss against composite_ref.nerf_loss64 on the
    part's own rgb and opacity with the ONE colour st.bg."""
    c, Np = st.cfg, st.Np
    bg = st.bg.cpu().double()
    total = 0.0
    for q, t in enumerate(st.parts):
        gt = batch.rgb[q * Np:(q + 1) * Np].cpu()
        l64, c64, o64 = R.nerf_loss64(t.rgb.cpu(), t.opacity.cpu(), gt, c.n_rays, c.lambda_opacity, bg)
        ec, eo = R.err(t.dL_drgb.cpu(), c64), R.err(t.dL_dop.cpu(), o64)
        e_max = float((t.rgb.cpu().double() + bg[None] * (1 - t.opacity.cpu().double())[:, None] - gt.double()).abs().max())
        print(f"{what} part {q}: E dL_drgb {ec:.3e} dL_dopacity {eo:.3e} (tolerance {16 * EPS:.3e}); max|e| {e_max:.3f}, "
              f"mean opacity {float(t.opacity.mean()):.3f}")
        assert ec <= 16 * EPS and eo <= 16 * EPS
        total += float(l64)
    # the NeRF loss: the fused kernel's partial sums, or (unfused route) the atomics' slot 0
    got = float(st._loss_acc[0]) if c.lambda_distortion > 0 else float(st.loss_sum)
    tol = 64 * EPS * abs(total) + 8 * EPS * abs(total)
    print(f"{what}: |loss - ref| {abs(got - total):.3e} (tolerance {tol:.3e}), loss {total:.5f}")
    assert abs(got - total) <= tol


@pytest.mark.parametrize("variant", ["fused", "two_parts", "distortion"])
def test_engine_eager_step_with_a_given_and_a_drawn_colour(gpu, variant):
    kw = {"fused": {}, "two_parts": dict(n_parts=2), "distortion": dict(lambda_distortion=1e-3)}[variant]
    on, off = _real_step(gpu, random_bg=True, **kw), _real_step(gpu, **kw)
    assert hasattr(on.mbuf[0], "bg") and not hasattr(off.mbuf[0], "bg")
    batch, noise = _given(gpu, on)
    # --- the colour (0, 0, 0) is the black of the step without the option, bit for bit
    for st, extra in ((on, dict(bg=(0.0, 0.0, 0.0))), (off, {})):
        st.run(batch, noise=noise, optimize=False, **extra)
    torch.cuda.synchronize()
    assert int(on.live_samples()) > 256 and on.skipped_steps() == 0
    assert torch.equal(on.bg, torch.zeros(3, device=gpu)) and torch.equal(off.bg, torch.zeros(3, device=gpu))
    for q, (a, b) in enumerate(zip(on.parts, off.parts)):
        n = int(on.state.counters[q, 0])  # the live samples (the buffers are sized for the worst case)
        assert n == int(off.state.counters[q, 0]) and n > 0
        for k in ("rgb", "opacity", "dL_drgb", "dL_dop"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        for k in ("dsig", "drgb_s"):
            assert torch.equal(getattr(a, k)[:n], getattr(b, k)[:n]), k
    if variant != "distortion":  # (that route's loss value is summed by float atomics in arrival order)
        assert torch.equal(on.loss_parts, off.loss_parts)
    # (several parts share the table gradient through float atomics, whose order is free: there the
    # per-ray and per-sample values above are the bit-for-bit statement)
    if variant != "two_parts":
        assert torch.equal(on.grads, off.grads) and float(on.grads.abs().max()) > 0
        on2, off2 = _real_step(gpu, random_bg=True, **kw), _real_step(gpu, **kw)
        p0 = on2.params.clone()
        on2.run(batch, noise=noise, bg=(0.0, 0.0, 0.0))
        off2.run(batch, noise=noise)
        torch.cuda.synchronize()
        for x, y in zip(_field_state(on2), _field_state(off2)):
            assert torch.equal(x, y)
        assert not torch.equal(on2.params, p0)
    # --- a drawn colour (the step's generator, after the noise) against fp64 with st.bg
    st = _real_step(gpu, random_bg=True, **kw)
    st.run(batch, noise=noise, optimize=False)
    torch.cuda.synchronize()
    drawn = st.bg.clone()
    assert st.bg.data_ptr() == st.mbuf[0].bg.data_ptr()
    assert bool((drawn >= 0).all()) and bool((drawn < 1).all()) and float(drawn.max()) > 0
    _check_parts_against_fp64(st, batch, f"{variant} drawn colour {[round(v, 4) for v in drawn.tolist()]}")
    # the colour reaches the gradient (the same step over black differs) and a given one replaces the draw
    assert not torch.equal(st.parts[0].dL_drgb, off.parts[0].dL_drgb)
    st.run(batch, noise=noise, optimize=False, bg=(0.25, 0.5, 0.75))
    torch.cuda.synchronize()
    assert st.bg.tolist() == [0.25, 0.5, 0.75]
    _check_parts_against_fp64(st, batch, f"{variant} given colour")


def test_engine_flag_is_ignored_on_a_synthetic_scene(gpu):
    """scale <= 0.5: accepted and ignored -- no buffer, the white constant, the bits of the step without."""
    mk = lambda **kw: engine.TrainStep(engine.StepConfig(n_rays=256, log2_T=14, **kw), device=gpu, seed=0)  # noqa: E731
    on, off = mk(random_bg=True), mk()
    for st in (on, off):
        st.set_occupancy(synthetic.ball_density_grid())
    batch, noise = _given(gpu, on)
    for st in (on, off):
        for _ in range(2):
            st.run(batch, noise=noise)
    torch.cuda.synchronize()
    assert not hasattr(on.mbuf[0], "bg") and on.bg.tolist() == [1.0, 1.0, 1.0]
    for x, y in zip(_field_state(on), _field_state(off)):
        assert torch.equal(x, y)
    assert torch.equal(on.gen.get_state(), off.gen.get_state())   # nothing new was drawn


def test_engine_generator_stream_is_unchanged_with_the_option_off(gpu):
    """random_bg off draws nothing new: the noise of two steps is the noise of the same generator
    without the option; on, three more values are drawn after each step's noise."""
    off, on = _real_step(gpu), _real_step(gpu, random_bg=True)
    batch, _ = _given(gpu, off)
    ref = torch.Generator(device=gpu)
    ref.manual_seed(1)  # TrainStep(seed=0) seeds its generator with seed + 1
    n0, c0 = torch.rand(256, generator=ref, device=gpu), torch.rand(3, generator=ref, device=gpu)
    off.run(batch)
    on.run(batch)
    torch.cuda.synchronize()
    assert torch.equal(on.state.noise, n0) and torch.equal(on.bg, c0)
    assert torch.equal(off.state.noise, n0)
    ref.manual_seed(1)
    torch.rand(256, generator=ref, device=gpu)
    n1 = torch.rand(256, generator=ref, device=gpu)
    off.run(batch)
    torch.cuda.synchronize()
    assert torch.equal(off.state.noise, n1)


# -------------------------------------------------------------------------------------- replay
@pytest.fixture(scope="module")
def views32(gpu):
    """12 analytic 32x32 views of the balls the occupancy prior marks (shared, never modified)."""
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    return data.ball_scene_views(data.BallScene.matching_grid(), 12, W, focal, seed=0, device=gpu)


SEED = 5


def _attached(gpu, views, **kw):
    imgs, poses, dirs, _ = views
    st = _real_step(gpu, random_bg=True, **kw)
    st.attach_dataset(data.DeviceDataset(imgs, poses, dirs, device=gpu, seed=SEED))
    return st


def _colour_is(st, k):
    got, want = st.bg.cpu().numpy(), B.bg_colour(SEED, k)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, got, want)


@pytest.mark.parametrize("refine", [False, True])
def test_replayed_step_trains_with_the_colour_of_its_own_batch(gpu, views32, refine):
    """Six steps: step k's colour is bg_colour(seed, k) -- k draws were made before its batch's -- eagerly
    and replayed, where the draw of step k+1 has already run (and written ITS colour into the other
    buffer set) when step k's colour is read back.  Eager and replayed parameters are the same bits."""
    kw = dict(refine_poses=True, pose_lr=0.0) if refine else {}
    a, b = _attached(gpu, views32, **kw), _attached(gpu, views32, **kw)
    for k in range(6):
        a.run()
        torch.cuda.synchronize()
        _colour_is(a, k)
    b.run()
    torch.cuda.synchronize()
    _colour_is(b, 0)
    b.capture()
    for k in range(1, 6):
        b.replay()
        torch.cuda.synchronize()
        _colour_is(b, k)
        # the batch drawn ahead carries its own colour with it, in the other set
        other = b.mbuf[1 - b.mbuf.index(b.state.march)].bg.cpu().numpy()
        assert np.array_equal(other.view(np.uint32), B.bg_colour(SEED, k + 1).view(np.uint32))
        assert int(b.dataset.calls[0]) == k + 2
    assert int(a.live_samples()) > 256
    for x, y in zip(_field_state(a), _field_state(b)):
        assert torch.equal(x, y)
    assert a.skipped_steps() == 0 and b.skipped_steps() == 0
    assert b.gate_timeouts() == 0
    if refine:
        assert float(b.dR.abs().max()) == 0 and float(b.pose_grad.abs().max()) > 0


def test_replay_with_staged_colours(gpu):
    """No dataset, capture(host_noise=True): replay(bg=, next_bg=) stages the colours like the noise; three
    replayed steps give the bits of the same three eager steps."""
    a, b = _real_step(gpu, random_bg=True), _real_step(gpu, random_bg=True)
    batches = a.make_batches(4, seed=2)
    g = torch.Generator().manual_seed(9)
    noise = [torch.rand(256, generator=g).to(gpu) for _ in range(4)]
    cols = [tuple(torch.rand(3, generator=g).tolist()) for _ in range(4)]
    for k in range(4):
        a.run(batches[k], noise=noise[k], bg=cols[k])
    b.run(batches[0], noise=noise[0], bg=cols[0])
    b.capture(host_noise=True)
    for k in range(1, 4):
        nxt = k + 1 < 4
        b.replay(batches[k], noise=noise[k], bg=cols[k], next_batch=batches[k + 1] if nxt else None,
                 next_noise=noise[k + 1] if nxt else None, next_bg=cols[k + 1] if nxt else None)
        torch.cuda.synchronize()
        assert b.bg.tolist() == list(torch.tensor(cols[k]).tolist())
    for x, y in zip(_field_state(a), _field_state(b)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="next_bg"):
        b.replay(batches[0], noise=noise[0])


# ------------------------------------------------------------------------------------- trainer
def _trainer(gpu, views, **kw):
    from mfnerf.trainer import HParams, Trainer
    imgs, poses, dirs, K = views
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(32, 32), device=gpu, seed=SEED)
    tr = Trainer(HParams(batch_size=256, T=14, num_epochs=1, steps_per_epoch=20, **kw), ds, device=gpu)
    tr.fit(log_every=0)
    torch.cuda.synchronize()
    return tr


def test_trainer_random_bg_trains_and_logs_the_psnr_of_its_loss(gpu, views32):
    from mfnerf.trainer import psnr
    tr = _trainer(gpu, views32, random_bg=True, scale=1.0)
    st = tr.step
    assert tr.global_step == 20 and st.skipped_steps() == 0 and st.gate_timeouts() == 0
    assert torch.isfinite(st.params).all()
    _colour_is(st, 19)                       # one draw per step, none for the occupancy refreshes
    m = tr.train_metrics()
    pred = torch.cat([t.rgb + st.bg[None] * (1 - t.opacity)[:, None] for t in st.parts])
    assert m["psnr"] == psnr(pred, st.last_batch.rgb)
    black = psnr(torch.cat([t.rgb for t in st.parts]), st.last_batch.rgb)
    print(f"trainer random_bg: psnr {m['psnr']:.3f} with st.bg, {black:.3f} over black; loss {m['loss']:.5f}")
    assert m["psnr"] != black and math.isfinite(m["loss"])
    # the logged PSNR is that of the loss the step minimised: loss = mse + lambda_opacity * entropy term
    o = torch.cat([t.opacity for t in st.parts]) + 1e-10
    want = float(((pred - st.last_batch.rgb) ** 2).mean() + st.cfg.lambda_opacity * (-o * torch.log(o)).mean())
    # (two fp32 sums of 768 + 256 terms in different orders: each within 1024 * 2^-24 = 6e-5 relative)
    assert abs(m["loss"] - want) <= 1.2e-4 * abs(want)


def test_trainer_flag_on_a_synthetic_scene_changes_nothing(gpu, views32):
    on, off = _trainer(gpu, views32, random_bg=True), _trainer(gpu, views32)
    assert on.step.skipped_steps() == 0
    for x, y in zip(_field_state(on.step), _field_state(off.step)):
        assert torch.equal(x, y)
    assert on.step.bg.tolist() == [1.0, 1.0, 1.0]
