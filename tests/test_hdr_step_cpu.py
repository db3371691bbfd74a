"""The HDR/exposure option of the fused step (StepConfig(hdr=True), Trainer(HParams(use_exposure=True)))
without a GPU: the guards, the dataset's exposures, and the step's host schedule recorded by
tools/launch_trace.py's Recorder (TrainStep on the CPU, library calls replaced by recorders)."""
import importlib.util
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
launch_trace = importlib.util.module_from_spec(spec)
spec.loader.exec_module(launch_trace)

HDR_CALLS = ("mfnerf_field_fw_lograd", "mfnerf_expand_exposure", "mfnerf_tonemap_fw_live", "mfnerf_tonemap_bw_live",
             "mfnerf_tonemap_unit_loss", "mfnerf_field_bw_lograd", "mfnerf_field_bw_inputs_lograd",
             "mfnerf_side_adam_step")


def _dataset(exposure=True, n=6, hw=64):
    from mfnerf.data import DeviceDataset
    gen = torch.Generator().manual_seed(0)
    kw = dict(exposure=torch.tensor([0.25, 1.0, 4.0] * (n // 3)), unit_exposure_rgb=0.73) if exposure else {}
    return DeviceDataset(torch.rand(n, hw, 3, generator=gen), torch.eye(4)[:3].repeat(n, 1, 1),
                         torch.rand(hw, 3, generator=gen), device="cpu", **kw)


# ---------------------------------------------------------------------------- data
def test_device_dataset_carries_exposures():
    from mfnerf.data import DeviceDataset
    ds = _dataset()
    assert ds.exposure.shape == (6,) and ds.exposure.dtype == torch.float32 and ds.unit_exposure_rgb == 0.73
    plain = _dataset(exposure=False)
    assert plain.exposure is None and plain.unit_exposure_rgb is None
    with pytest.raises(ValueError, match="exposure"):
        DeviceDataset(torch.zeros(2, 4, 3), torch.zeros(2, 3, 4), torch.zeros(4, 3), device="cpu",
                      exposure=torch.ones(3))
    src = types.SimpleNamespace(rays=torch.zeros(2, 4, 3), poses=torch.zeros(2, 3, 4), directions=torch.zeros(4, 3),
                                K=None, img_wh=None, exposure=torch.tensor([0.5, 2.0]), unit_exposure_rgb=0.5)
    got = DeviceDataset.from_dataset(src, device="cpu")
    assert torch.equal(got.exposure, src.exposure) and got.unit_exposure_rgb == 0.5
    del src.exposure, src.unit_exposure_rgb
    assert DeviceDataset.from_dataset(src, device="cpu").exposure is None


def test_analytic_hdr_scene():
    from mfnerf.data import HDR_EXPOSURES, BallScene, ball_scene_views, camera_response, hdr_ball_scene_views
    scene = BallScene(n_balls=6, seed=1)
    imgs, poses, dirs, K, exposure = hdr_ball_scene_views(scene, 2, 16, 20.0, seed=3)
    E = len(HDR_EXPOSURES)
    assert E >= 3 and imgs.shape == (2 * E, 256, 3) and poses.shape == (2 * E, 3, 4) and exposure.shape == (2 * E,)
    assert exposure.tolist() == list(HDR_EXPOSURES) * 2
    ldr = ball_scene_views(scene, 2, 16, 20.0, seed=3)[0]
    for i in range(2 * E):
        assert torch.equal(poses[i], poses[i // E * E])
        rad = ldr[i // E]
        hit = (rad != 1).any(-1)  # the balls' colours stay below 0.9
        assert 0 < int(hit.sum()) < 256
        assert torch.equal(imgs[i][~hit], torch.ones(int((~hit).sum()), 3)), "white background at every exposure"
        assert torch.allclose(imgs[i][hit], camera_response(rad[hit] * exposure[i]))
    assert float(camera_response(torch.tensor(4.0))) == 1.0 and float(camera_response(torch.tensor(-1.0))) == 0.0


# ---------------------------------------------------------------------------- guards
def test_step_config_defaults_are_off():
    from mfnerf import engine
    c = engine.StepConfig()
    assert c.hdr is False and c.unit_exposure_rgb == 0.5
    assert engine.Batch(None, None, None).exposure is None


def test_trainer_guards():
    from mfnerf import trainer
    hp = trainer.HParams(use_exposure=True)
    for train in (None, _dataset(exposure=False)):
        with pytest.raises(NotImplementedError, match="HDR/exposure"):
            trainer.Trainer(hp, train, device="cpu")
    with pytest.raises(NotImplementedError, match="one GPU"):
        trainer.Trainer(hp, _dataset(), device="cpu", world=2)


@pytest.fixture()
def rec(monkeypatch):
    r = launch_trace.Recorder()
    r.install(monkeypatch.setattr)
    return r


def _step(rec, **kw):
    from mfnerf import engine
    cfg = engine.StepConfig(**{**launch_trace.BASE, "hdr": True, "unit_exposure_rgb": 0.73, **kw})
    rec.step = engine.TrainStep(cfg, device="cpu")
    return rec.step


def test_step_guards(rec):
    from mfnerf import dp, engine
    with pytest.raises(ValueError, match="hdr needs n_parts == 1"):
        _step(rec, n_parts=2)
    st = _step(rec)
    assert st.tm_params.shape == (3, 2048) and st.tm_grad.shape == st.tm_m.shape == st.tm_v.shape == (3, 2048)
    assert int(st.tm_step_dev) == 0 and st.loss_parts.numel() == st._nb_part + 64 + 3
    with pytest.raises(ValueError, match="sharded optimizer"):
        st.shard_optimizer(0, 2)
    b = st.make_batches(1)[0]
    with pytest.raises(ValueError, match="exposure"):
        st.run(b)
    b.exposure = torch.ones(st.cfg.n_rays)
    with pytest.raises(ValueError, match="gradient exchange"):
        st.run(b, exchange=dp.allreduce_mean_)
    st.run(b)
    st.attach_dataset(_dataset(exposure=False))
    with pytest.raises(ValueError, match="per-image exposures"):
        st.run()
    # off: no tonemapper state, the loss slots of before
    off = engine.TrainStep(engine.StepConfig(**launch_trace.BASE), device="cpu")
    assert off.tm_params is None and off.loss_parts.numel() == off._nb_part + 64
    assert not hasattr(off.parts[0], "lograd") and not hasattr(off.mbuf[0], "exposure")


def test_init_leaves_the_ldr_draws_alone(rec):
    """The tonemappers are drawn after the field's parameters from the same seeded generator."""
    from mfnerf import engine
    st = _step(rec)
    off = engine.TrainStep(engine.StepConfig(**launch_trace.BASE), device="cpu")
    assert torch.equal(st.params, off.params)
    tm = engine.init_tonemappers(st.cfg, st.n_params, st.n_alloc, 0)
    assert torch.equal(tm, st.tm_params)
    lim = (6.0 / 80) ** 0.5
    assert float(tm.abs().max()) <= lim and float(tm.abs().max()) > 0.9 * lim
    assert not torch.equal(tm[0], tm[1])


# ---------------------------------------------------------------------------- the schedule
def _trace(rec, dataset, **kw):
    st = _step(rec, **kw)
    b = [None] * 3
    if dataset:
        st.attach_dataset(_dataset())
    else:
        b = st.make_batches(3)
        for i, x in enumerate(b):
            x.exposure = torch.full((st.cfg.n_rays,), 0.5 + i)
    rec.extra_roots = [b]
    with rec.torch_ops():
        for i in range(2):
            rec.phase(f"run{i}")
            st.run(b[0])
        rec.phase("capture")
        st.capture()
        for i in range(3):
            rec.phase(f"replay{i}")
            st.replay(b[i % 3], next_batch=b[(i + 1) % 3])
        rec.phase("run_no_optimize")
        st.run(b[0], optimize=False)
    return rec.document()


def _phase(events, name):
    names = [e.get("name") if e["op"] == "phase" else None for e in events]
    a = names.index(name)
    b = next((i for i in range(a + 1, len(events)) if events[i]["op"] == "phase"), len(events))
    return events[a + 1:b]


def _names(events):
    return [e["name"] for e in events if e["op"] == "call"]


def _check_order(names, bw="mfnerf_field_bw_lograd", composite=("mfnerf_composite_train_fused",)):
    i = {n: names.index(n) for n in set(names)}
    assert names.count("mfnerf_side_adam_step") == 1 and "mfnerf_field_fw" not in i and "mfnerf_field_bw" not in i
    comp = [i[c] for c in composite]
    assert i["mfnerf_grid_encode_fw_planar"] < i["mfnerf_field_fw_lograd"] < i["mfnerf_expand_exposure"] \
        < i["mfnerf_tonemap_fw_live"] < min(comp)
    assert max(comp) < i["mfnerf_tonemap_bw_live"] < i["mfnerf_tonemap_unit_loss"] < i[bw] < i["mfnerf_side_adam_step"]
    main = [k for k, n in enumerate(names) if "adam" in n and n != "mfnerf_side_adam_step"]
    if main:  # the main optimizer call (it clears the non-finite flag) comes after the side Adam
        assert i["mfnerf_side_adam_step"] < min(main)


def _exposure_buffers(events):
    """(buffers the expansion reads its per-ray exposure from, buffers a torch op filled before it)."""
    read = [e["args"][0][0] for e in events if e["op"] == "call" and e["name"] == "mfnerf_expand_exposure"]
    return read


@pytest.mark.parametrize("dataset", [True, False], ids=["dataset", "batches"])
def test_schedule(rec, dataset):
    ev = _trace(rec, dataset)
    caps = {e["graph"]: e["events"] for e in ev if e["op"] == "capture"}
    eager = _phase(ev, "run1")
    _check_order(_names(eager))
    assert any("adam" in n and n != "mfnerf_side_adam_step" for n in _names(eager))
    for j in range(2):
        _check_order(_names(caps[f"chain[{j}][0]"]))
        _check_order(_names(caps[f"step[{j}]"]))
        assert any("adam" in n and n != "mfnerf_side_adam_step" for n in _names(caps[f"step[{j}]"]))
    # optimize=False: the backward's gradients stay, neither optimizer runs
    held = _names(_phase(ev, "run_no_optimize"))
    assert "mfnerf_tonemap_unit_loss" in held and not any("adam" in n for n in held)
    # the per-ray exposure the chain reads is the buffer the batch's draw / staging filled in the march
    # buffer set it trains on: eager set 0; captured, set j's march graph (dataset) or the copy that
    # replay() issues before it (batches)
    op = "aten.index_select.out" if dataset else "aten.copy_.default"

    def filled(events):
        return [e["dst"][0] for e in events if e["op"] == "torch" and e["name"] == op]

    (e_read,) = set(_exposure_buffers(eager))
    assert e_read in filled(eager)
    sets = []
    for j in range(2):
        (r_chain,) = set(_exposure_buffers(caps[f"chain[{j}][0]"]))
        (r_step,) = set(_exposure_buffers(caps[f"step[{j}]"]))
        assert r_chain == r_step
        sets.append(r_chain)
        if dataset:
            for g in (f"march[{j}]", f"march_gated[{j}]"):
                assert filled(caps[g]) == [r_chain], g
    assert sets[0] != sets[1] and sets[0] == e_read
    if not dataset:  # replay k stages batch k's exposure into set k % 2 ... and the next batch's into the other
        r0 = filled(_phase(ev, "replay0"))
        assert sets[0] in r0 and sets[1] in r0
    # the expansion reads the rays_a and the device counter of the same set as its exposure
    for j in range(2):
        (c,) = [e for e in caps[f"step[{j}]"] if e["op"] == "call" and e["name"] == "mfnerf_expand_exposure"]
        (m,) = [e for e in caps[f"march[{j}]"] if e["op"] == "call" and e["name"] == "mfnerf_raymarching_train"]
        assert c["args"][1] == m["args"][13] and c["args"][4] == m["args"][18]


def test_schedule_distortion_random_bg_and_ray_grads(rec):
    """Both loss forms, random_bg and the _inputs_lograd backward take the same places."""
    ev = _trace(rec, True, lambda_distortion=1e-3, random_bg=True, scale=4.0, ray_grads=True)
    names = _names(_phase(ev, "run1"))
    _check_order(names, bw="mfnerf_field_bw_inputs_lograd",
                 composite=("mfnerf_composite_train_fw", "mfnerf_nerf_loss_bg", "mfnerf_composite_train_bw"))
    assert "mfnerf_sample_rays_prep_bg" in names and "mfnerf_rays_input_grad" in names


def test_off_means_no_hdr_launch(monkeypatch):
    ev = launch_trace.trace(("default",), setattr_=monkeypatch.setattr)["default"]

    def flat(events):
        for e in events:
            yield e
            yield from flat(e.get("events", ()))
    names = {e["name"] for e in flat(ev) if e["op"] == "call"}
    assert names and not names & set(HDR_CALLS)
