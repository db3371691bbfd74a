"""The HDR/exposure model inside the fused training step (StepConfig(hdr=True),
Trainer(HParams(use_exposure=True))) on the analytic HDR scene (mfnerf.data.hdr_ball_scene_views: three
exposures per pose), n_rays = 1024, log2_T = 15.

* one eager step, stage by stage from the step's own upstream buffers against the fp64 references
  (tests/field_hdr_ref.py, tests/tonemap_ref.py) under the kernel tests' bounds -- the method of
  test_distortion_loss_in_the_fused_step;
* the step's loss against the module route (NGP('None') with the same weights, render() with the same
  noise, NeRFLoss, the unit-exposure term) at test_gpu_configs.py's 1e-4 relative, on condition that
  the module route run on row-major and on planar features differs from itself by less than a third
  of that (measured and printed);
* a captured, pipelined replay of six steps with an attached dataset, bit for bit the eager steps;
* an injected non-finite gradient skips the field's and the tonemappers' update together;
* Trainer(HParams(use_exposure=True)) for 256 steps: the loss falls, the train-exposure PSNR of
  to_ngp() is not below the module route's (render() + autograd + torch Adam, the same steps from the
  same init) by more than three standard deviations of the module route's own PSNR over three seeds
  (measured here and printed); the checkpoint round trip with the tonemappers' keys; evaluate(exposures=).

Measured on an MI355X: log-radiance error 2.4e-4 at |log-radiance| <= 0.57; rgb_s at 0.21 of its bound,
dlograd at 1.5e-4, tm_grad at 0.52 (60 of 34,453 samples on a kink); dL_dfeat 2.4e-4, gx 9.4e-8,
gr 1.0e-6 of the maximum (bound 2e-3); step loss against the module route 5.8e-8 relative, the module
route's row-major / planar self-spread 0 (the two encoders give the same bits).  256 trainer steps:
loss 0.00592 -> 0.00022, train-exposure PSNR 37.76 dB fused against 38.16 dB for the module route from
the same init (seeds 38.16, 40.10, 37.56: std 1.33 dB, margin 3.98 dB).  Without the GradScaler the
module route's fp16 MLP backward underflows and it reaches 28.8-33.0 dB.
"""
import functools
import math

import pytest
import torch

import field_hdr_ref as H
import tonemap_ref as TR
from mfnerf import data, engine
from mfnerf.field import XYZ_NET_PARAMS
from mfnerf.trainer import HParams, Trainer

pytestmark = pytest.mark.gpu

N_RAYS, LOG2_T, W_IMG, UNIT = 1024, 15, 48, data.UNIT_EXPOSURE_RGB_SYNTHETIC
FOCAL = 0.5 * W_IMG / math.tan(0.5 * 0.6911112)
TOL = 2e-3  # test_field_bw: max error / max reference


@functools.lru_cache(maxsize=None)
def _scene():
    """The analytic HDR scene: 16 poses x 3 exposures of 48 x 48 pixels (computed once, left unchanged)."""
    sc = data.BallScene(n_balls=6, seed=1)
    imgs, poses, dirs, K, exposure = data.hdr_ball_scene_views(sc, 16, W_IMG, FOCAL, seed=0)
    assert len(set(exposure.tolist())) >= 3
    return sc, imgs, poses, dirs, K, exposure


def _dataset(gpu, seed=5):
    _, imgs, poses, dirs, K, exposure = _scene()
    return data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W_IMG, W_IMG), device=gpu, seed=seed, exposure=exposure,
                              unit_exposure_rgb=UNIT)


def _step(gpu, **kw):
    st = engine.TrainStep(engine.StepConfig(n_rays=N_RAYS, log2_T=LOG2_T, hdr=True, unit_exposure_rgb=UNIT, **kw),
                          device=gpu, seed=0)
    st.set_occupancy(_scene()[0].density_grid())
    return st


def _batches(gpu, k, seed=5):
    """k explicit batches drawn from the dataset, each with its rays' exposures."""
    ds = _dataset(gpu, seed)
    out = []
    for _ in range(k):
        buf = torch.empty(3, N_RAYS, 3, device=gpu)
        ii, pp = torch.empty(N_RAYS, dtype=torch.int32, device=gpu), torch.empty(N_RAYS, dtype=torch.int32, device=gpu)
        ds.sample(buf, ii, pp)
        out.append(engine.Batch(buf[0], buf[1], buf[2], buf, exposure=ds.exposure[ii.long()].contiguous()))
    return out


def _noise(gpu, seed):
    return torch.rand(N_RAYS, generator=torch.Generator().manual_seed(seed)).to(gpu)


def _model(st):
    """NGP('None') holding the step's weights (what Trainer.to_ngp builds)."""
    from mfnerf.networks import NGP
    c = st.cfg
    hp = HParams(scale=c.scale, T=c.log2_T, batch_size=c.n_rays, rgb_channels=c.rgb_width)
    m = NGP(scale=c.scale, hparams=hp, rgb_act="None").to(st.dev)
    with torch.no_grad():
        p = st.params
        m.xyz_encoder.params.copy_(torch.cat([p[:XYZ_NET_PARAMS], p[st.off_table:st.n_params]]))
        m.rgb_net.params.copy_(p[st.off_rgb:st.off_table])
        m.density_grid.copy_(st.density_grid)
        m.density_bitfield.copy_(st.bitfield)
        for i in range(3):
            getattr(m, f"tonemapper_net_{i}").params.copy_(st.tm_params[i])
    return m


def _cpu(t):
    return t.detach().cpu()


# ---------------------------------------------------------------------------- one step, stage by stage
WARM = 2  # updates before the inspected step: the weights have left their init, and the log-radiance is
          # still below 4, where one fp16 step (2^-9) is inside test_field_fw's atol (asserted below)


@functools.lru_cache(maxsize=None)
def _inspected():
    """A step after WARM updates, run with optimize=False: its buffers on the host."""
    gpu = torch.device("cuda:0")
    st = _step(gpu)
    b = _batches(gpu, WARM + 1)
    for k in range(WARM):
        st.run(b[k], noise=_noise(gpu, k))
    st.run(b[WARM], noise=_noise(gpu, WARM), optimize=False)
    torch.cuda.synchronize()
    assert st.skipped_steps() == 0 and int(st.tm_step_dev) == WARM and int(st.step_dev) == WARM
    t, m = st.parts[0], st.state.march.part[0]
    n = int(m.counter[0])
    assert n > 10 * N_RAYS
    feat = t.feat[:, :n].permute(1, 0, 2).reshape(n, 32)
    p = _cpu(st.params)
    r = dict(st=st, n=n, batch=b[WARM], feat=_cpu(feat), dirs=_cpu(m.dirs[:n]), rays_a=_cpu(m.rays_a),
             px=p[:XYZ_NET_PARAMS], pr=p[st.off_rgb:st.off_table], tm=_cpu(st.tm_params).reshape(-1),
             sigma=_cpu(t.sigma[:n]), lograd=_cpu(t.lograd[:n]), exposure_s=_cpu(t.exposure_s[:n]),
             rgb_s=_cpu(t.rgb_s[:n]), dsig=_cpu(t.dsig[:n]), drgb_s=_cpu(t.drgb_s[:n]), dlograd=_cpu(t.dlograd[:n]),
             dfeat=_cpu(t.dfeat[:n]), tm_grad=_cpu(st.tm_grad).reshape(-1), grads=_cpu(st.grads[:st.off_table]),
             exposure=_cpu(st.state.march.exposure), S=st.loss_scale(), loss_unit=_cpu(st._loss_unit))
    return r


def test_stage_lograd_from_feat(gpu):
    r = _inspected()
    s_ref, l_ref, _ = H.forward(r["feat"], r["dirs"], r["px"], r["pr"], 64)
    assert r["lograd"].dtype == torch.float16
    # test_field_fw's bounds
    assert torch.allclose(r["sigma"].double(), s_ref, rtol=4e-3, atol=1e-6)
    err = float((r["lograd"].double() - l_ref).abs().max())
    print(f"n={r['n']}: log-radiance max error {err:.3e} (max |ref| {float(l_ref.abs().max()):.3f})")
    assert float(l_ref.abs().max()) < 4, "one fp16 step of the log-radiance would exceed the bound"
    assert torch.allclose(r["lograd"].double(), l_ref, atol=2e-3, rtol=0)


def test_stage_rgb_from_lograd_and_exposure(gpu):
    r = _inspected()
    ra = r["rays_a"]
    want_e = torch.repeat_interleave(r["exposure"][ra[:, 0]], ra[:, 2], 0)
    assert torch.equal(r["exposure_s"], want_e) and len(set(want_e.tolist())) >= 3
    assert torch.equal(r["exposure"], r["batch"].exposure.cpu())
    f = TR.forward(r["lograd"], r["exposure_s"], r["tm"])
    err = (r["rgb_s"].double() - f["y"]).abs()
    bound = 2.0 ** -10 + 2.0 ** -13 * f["B"]
    print("rgb_s max err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    assert torch.equal(r["rgb_s"], r["rgb_s"].half().float()), "fp32 holding the half value"


def test_stage_dlograd_and_tm_grad_from_drgb(gpu):
    from mfnerf import tonemap
    r = _inspected()
    n = r["n"]
    f = TR.forward(r["lograd"], r["exposure_s"], r["tm"])
    keep = ~f["kink"]
    assert int(f["kink"].sum()) <= 0.01 * n, "too many samples on a ReLU kink for this comparison"
    b = TR.backward(r["lograd"], r["exposure_s"], r["tm"], r["rgb_s"], r["drgb_s"], keep=keep)
    err = (r["dlograd"].double() - b["dx"]).abs()[keep]
    bound = ((2.0 ** -9 + 64 * 2.0 ** -23) * b["A_s"])[keep]
    print("dlograd max err/bound", float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all())
    # the samples on a kink: their gate may fall either way, so their whole terms go into the bound
    b_all = TR.backward(r["lograd"], r["exposure_s"], r["tm"], r["rgb_s"], r["drgb_s"])
    A_kink = b_all["A"] - b["A"]
    # the unit-exposure term, from the kernel's own half output at log-radiance 0
    zero = torch.zeros(1, 3).half()
    y16 = tonemap.tonemap_fw(zero.to(gpu), None, 0, r["tm"].to(gpu)).cpu()
    u = TR.backward(zero, None, r["tm"], y16, (y16.double() - UNIT) / 3)
    ref = b["g"] + u["g"]
    gbound = (2.0 ** -9 + n * 2.0 ** -23) * b["A"] + A_kink + (2.0 ** -9 + 2.0 ** -23) * u["A"] \
        + 2.0 ** -23 * (b["g"].abs() + u["g"].abs())
    gerr = (r["tm_grad"].double() - ref).abs()
    print("tm_grad max err/bound", float((gerr / gbound.clamp(min=1e-300)).max()),
          "kink samples", int(f["kink"].sum()), "unit share of |grad|", float(u["g"].abs().max() / ref.abs().max()))
    assert bool((gerr <= gbound).all()) and float(ref.abs().max()) > 0
    want = (0.5 * (y16.double() - UNIT) ** 2 / 3).reshape(3)
    assert torch.allclose(r["loss_unit"].double(), want, rtol=1e-5, atol=0)


def test_stage_mlp_gradients_from_dlograd(gpu):
    r = _inspected()
    _, _, acts = H.forward(r["feat"], r["dirs"], r["px"], r["pr"], 64)
    ref = H.backward(acts, r["dsig"], r["dlograd"], r["S"])
    got = (r["dfeat"], r["grads"][:XYZ_NET_PARAMS], r["grads"][XYZ_NET_PARAMS:])
    for name, g, w in zip(("dL_dfeat", "gx", "gr"), got, ref):
        err = float((g.double() - w).abs().max() / w.abs().max())
        print(f"{name}: max error / max reference {err:.3e}")
        assert err < TOL, (name, err)


# ---------------------------------------------------------------------------- loss vs the module route
def _module_loss(st, batch, noise, planar):
    """NGP('None') with the step's weights through render() with the given noise, NeRFLoss and the
    unit-exposure term (train.py:172-177).  planar: the grid features come from the planar encoder
    the step uses (level planes, transposed back) instead of the row-major one."""
    from mfnerf import rendering, tcnn
    from mfnerf._lib import call, ptr, stream
    from mfnerf.losses import NeRFLoss
    model = _model(st)
    enc = model.xyz_encoder
    if planar:
        def forward(x):
            n = x.shape[0]
            planes = torch.empty(16, n, 2, dtype=torch.float16, device=x.device)
            cnt = torch.tensor([n], dtype=torch.int32, device=x.device)
            call("mfnerf_grid_encode_fw_planar", ptr(x.float().contiguous()), n, ptr(cnt), 0.0, 1.0, enc.desc,
                 ptr(enc.params[enc.n_net:].detach().half()), ptr(planes), n, stream())
            feat = planes.permute(1, 0, 2).reshape(n, 32)
            return tcnn.mlp_forward(feat, enc.params[:enc.n_net], enc.width, enc.depth, enc.n_output_dims,
                                    enc.activation, enc.output_activation)
        enc.forward = forward
    real = torch.rand_like
    torch.rand_like = lambda t, *a, **k: noise.clone() if t.shape == (N_RAYS,) else real(t, *a, **k)
    try:
        with torch.no_grad():
            res = rendering.render(model, batch.rays_o, batch.rays_d, exposure=batch.exposure.reshape(-1, 1))
    finally:
        torch.rand_like = real
    d = NeRFLoss(lambda_opacity=st.cfg.lambda_opacity, lambda_distortion=0)(res, {"rgb": batch.rgb})
    with torch.no_grad():
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=st.dev), exposure=torch.ones(1, 1, device=st.dev))
    return float(sum(v.double().mean() for v in d.values()) + (0.5 * (unit.double() - UNIT) ** 2).mean()), \
        int(res["rm_samples"])


def test_step_loss_vs_module_route(gpu):
    r = _inspected()
    st, batch = r["st"], r["batch"]
    noise = _noise(gpu, WARM)
    got = float(st.loss_sum)
    rows, n_rows = _module_loss(st, batch, noise, planar=False)
    plan, n_plan = _module_loss(st, batch, noise, planar=True)
    assert n_rows == n_plan == r["n"], "the module route marched other samples"
    spread = abs(rows - plan) / rows
    print(f"step loss {got:.8f}, module route {rows:.8f} (planar features {plan:.8f}): "
          f"relative difference {abs(got - rows) / rows:.3e}, module self-spread {spread:.3e}")
    assert spread < 1e-4 / 3, spread
    assert abs(got - rows) <= 1e-4 * rows, (got, rows)


# ---------------------------------------------------------------------------- replay
def _state(st):
    return (st.params, st.p16, st.m, st.v, st.tm_params, st.tm_m, st.tm_v, st.step_dev, st.tm_step_dev)


def test_captured_pipelined_replay_equals_eager(gpu):
    a, b = _step(gpu), _step(gpu)
    a.attach_dataset(_dataset(gpu))
    b.attach_dataset(_dataset(gpu))
    for _ in range(6):
        a.run()
    b.run()
    b.capture()
    for _ in range(5):
        b.replay()
    torch.cuda.synchronize()
    assert int(a.step_dev) == 6 and int(a.tm_step_dev) == 6 and a.skipped_steps() == 0 and b.skipped_steps() == 0
    assert int(a.live_samples()) > N_RAYS and b.gate_timeouts() == 0
    for name, x, y in zip("params p16 m v tm_params tm_m tm_v step_dev tm_step_dev".split(), _state(a), _state(b)):
        assert torch.equal(x, y), name
    assert float(a.tm_m.abs().max()) > 0
    assert torch.equal(a.loss_parts, b.loss_parts)


# ---------------------------------------------------------------------------- non-finite gradient
def test_nonfinite_gradient_skips_field_and_tonemappers_together(gpu):
    """As test_nonfinite_gradient_skips_the_step: the NaN enters through the loss target."""
    st = _step(gpu)
    bad, good = _batches(gpu, 2)
    bad.rgb.fill_(float("nan"))
    before = [t.clone() for t in _state(st)]
    st.run(bad)
    torch.cuda.synchronize()
    for name, x, y in zip("params p16 m v tm_params tm_m tm_v step_dev tm_step_dev".split(), before, _state(st)):
        assert torch.equal(x, y), name
    assert st.skipped_steps() == 1 and int(st.finite_status[0]) == 0
    st.run(good)
    torch.cuda.synchronize()
    assert not torch.equal(st.params, before[0]) and not torch.equal(st.tm_params, before[4])
    assert int(st.step_dev) == 1 and int(st.tm_step_dev) == 1 and st.skipped_steps() == 1
    assert torch.isfinite(st.params).all() and torch.isfinite(st.tm_params).all()


# ---------------------------------------------------------------------------- training quality
STEPS = 256
HP = dict(batch_size=N_RAYS, T=LOG2_T, use_exposure=True, num_epochs=1, steps_per_epoch=STEPS)


def _train_psnr(model, gpu, views=(0, 1, 2, 24, 25, 26)):
    """PSNR of the test-time render at the training exposures against the training images."""
    from mfnerf.rendering import render
    _, imgs, poses, dirs, _, exposure = _scene()
    vals = []
    with torch.no_grad():
        for i in views:
            o, d = data.get_rays(dirs.to(gpu), poses[i].to(gpu))
            res = render(model, o, d, test_time=True, exposure=exposure[i].to(gpu).reshape(1, 1))
            vals.append(float(-10 * torch.log10(((res["rgb"].float() - imgs[i].to(gpu)) ** 2).mean())))
    return sum(vals) / len(vals)


def _module_route_training(model, gpu, seed):
    """train.py's step module by module: the occupancy cadence, a batch from the dataset's draw,
    render() + NeRFLoss + the unit term, autograd under torch's GradScaler (PL precision=16,
    train.py:287: without it the fp16 MLP backward underflows), torch Adam(eps 1e-15) with the cosine
    schedule."""
    from mfnerf.losses import NeRFLoss
    from mfnerf.rendering import render
    from mfnerf.trainer import UPDATE_INTERVAL, WARMUP_STEPS, cosine_lr
    ds = _dataset(gpu)
    hp = HParams(**HP, seed=seed)
    opt = torch.optim.Adam([p for p in model.parameters() if p.numel()], lr=hp.lr, eps=1e-15)
    loss_fn = NeRFLoss(lambda_distortion=0)
    scaler = torch.amp.GradScaler("cuda")
    buf = torch.empty(3, N_RAYS, 3, device=gpu)
    ii, pp = torch.empty(N_RAYS, dtype=torch.int32, device=gpu), torch.empty(N_RAYS, dtype=torch.int32, device=gpu)
    for step in range(STEPS):
        if step % UPDATE_INTERVAL == 0:
            model.update_density_grid(engine.DENSITY_THRESHOLD, warmup=step < WARMUP_STEPS)
        for g in opt.param_groups:
            g["lr"] = cosine_lr(step // hp.steps_per_epoch, hp)
        ds.sample(buf, ii, pp)
        res = render(model, buf[0], buf[1], exposure=ds.exposure[ii.long()].reshape(-1, 1))
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=gpu), exposure=torch.ones(1, 1, device=gpu))
        loss = sum(v.mean() for v in loss_fn(res, {"rgb": buf[2]}).values()) + (0.5 * (unit.float() - UNIT) ** 2).mean()
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    return _train_psnr(model, gpu)


def test_trainer_use_exposure(gpu, tmp_path):
    ds = _dataset(gpu)
    tr = Trainer(HParams(**HP), ds, device=gpu)
    assert tr.step.cfg.hdr and tr.step.cfg.unit_exposure_rgb == UNIT
    init = tr.to_ngp()
    assert init.rgb_act == "None"
    hist = tr.fit(steps=STEPS, log_every=32)
    losses = [h["loss"] for h in hist]
    assert hist[-1]["skipped"] == 0 and int(tr.step.tm_step_dev) == STEPS
    assert losses[-1] < 0.5 * losses[0], losses
    fused = _train_psnr(tr.to_ngp(), gpu)
    # the module route from the same init, and from two more seeds' inits for its own spread
    module = [_module_route_training(init, gpu, HParams().seed)]
    for seed in (1, 2):
        other = Trainer(HParams(**HP, seed=seed), _dataset(gpu), device=gpu)
        module.append(_module_route_training(other.to_ngp(), gpu, seed))
        del other
    mean = sum(module) / 3
    std = (sum((m - mean) ** 2 for m in module) / 2) ** 0.5
    print(f"\nloss {losses[0]:.5f} -> {losses[-1]:.5f}; train-exposure PSNR fused {fused:.2f} dB, module route "
          f"{module[0]:.2f} dB (same init), seeds {[round(m, 2) for m in module]}: std {std:.3f} dB, margin {3 * std:.3f}")
    assert fused >= module[0] - 3 * std, (fused, module, std)
    # checkpoint round trip with the reference's tonemapper keys: fresh moments and step counts
    path = str(tmp_path / "hdr.ckpt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
    for i in range(3):
        assert torch.equal(sd[f"model.tonemapper_net_{i}.params"], tr.step.tm_params[i].cpu())
    tr2 = Trainer(HParams(**HP), _dataset(gpu), device=gpu)
    tr2.load(path)
    assert torch.equal(tr2.step.tm_params, tr.step.tm_params)
    assert torch.equal(tr2.step.p16[:tr.step.n_params], tr.step.p16[:tr.step.n_params])
    assert float(tr2.step.tm_m.abs().max()) == 0 and float(tr2.step.tm_v.abs().max()) == 0
    assert int(tr2.step.tm_step_dev) == 0 and int(tr2.step.step_dev) == 0
    # evaluate(exposures=) is render(test_time=True, exposure=) of to_ngp()
    _, imgs, poses, dirs, _, exposure = _scene()
    views = [1, 26]
    mean_psnr, per_view = tr.evaluate(imgs[views], poses[views], dirs, exposures=exposure[views])
    want = [_train_psnr(tr.to_ngp(), gpu, views=(i,)) for i in views]
    assert per_view == pytest.approx(want, abs=1e-9) and mean_psnr == pytest.approx(sum(want) / 2, abs=1e-9)
    v = tr.validate(imgs[views], poses[views], dirs, exposures=exposure[views])
    assert v["psnr_per_view"] == pytest.approx(want, abs=1e-3)
    unit_view, _ = tr.evaluate(imgs[views[:1]], poses[views[:1]], dirs)  # exposure 1: another image
    assert abs(unit_view - want[0]) > 1e-3 or float(exposure[views[0]]) == 1.0
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        tr.evaluate(imgs[views], poses[views], dirs, fused=True, exposures=exposure[views])
