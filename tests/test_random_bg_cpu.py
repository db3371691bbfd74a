"""CPU tests of --random_bg inside the fused step: the NumPy definition of the colour draw
(tests/bg_ref.py) as a random number generator, the three new entry points' declarations against
their ctypes signatures, and the configuration surface (StepConfig.random_bg, HParams.random_bg).
No GPU compute."""
import ctypes
import os

import numpy as np
import pytest

import bg_ref as B
from test_pose_refine_cpu import _NoInit, _declared_args

NEW_ENTRY_POINTS = ["mfnerf_composite_train_fused_bg", "mfnerf_nerf_loss_bg", "mfnerf_sample_rays_prep_bg"]
N_CALLS = 20000


def test_bg_colour_is_three_float32_in_unit_interval():
    for seed in (0, 5, 1337, 2 ** 63 + 11, -1):
        c = B.bg_colour(seed, 0)
        assert c.shape == (3,) and c.dtype == np.float32
        assert (c >= 0).all() and (c < 1).all()
    many = B.bg_colour(5, np.arange(N_CALLS))
    assert many.shape == (N_CALLS, 3) and many.dtype == np.float32
    assert (many >= 0).all() and (many < 1).all()
    assert np.array_equal(many[7], B.bg_colour(5, 7))           # the array form is the scalar form
    # 24 bits: every value is a multiple of 2^-24
    assert np.array_equal(many * np.float32(2.0 ** 24), np.floor(many * np.float32(2.0 ** 24)))


def test_bg_colour_differs_between_calls_and_seeds():
    a = [B.bg_colour(5, k) for k in range(6)]
    for k in range(5):
        assert not np.any(a[k] == a[k + 1]), k
    assert not np.any(B.bg_colour(5, 0) == B.bg_colour(6, 0))
    # its own stream: with the ray or noise draws' constant the values are others
    ref = B.bg_colour(5, 3)
    for other in (B.RAY_STREAM, B.NOISE_STREAM):
        key = B.splitmix64(B.splitmix64(np.uint64(5) ^ other) ^ np.uint64(3))
        with np.errstate(over="ignore"):
            v = (B.mix32(key + np.arange(3, dtype=np.uint64) * B.GOLDEN) >> np.uint32(8)).astype(np.float32) * 2.0 ** -24
        assert not np.any(v == ref)
    assert len({int(B.BG_STREAM), int(B.RAY_STREAM), int(B.NOISE_STREAM)}) == 3


def test_bg_colour_statistics_over_20000_calls():
    """Each component's mean within 0.01 of 0.5 (4.9 sigma of the mean of 20 000 uniforms, sigma =
    sqrt(1/12/20000) = 0.0020) and variance within 0.005 of 1/12; components pairwise uncorrelated and
    consecutive calls uncorrelated to |r| < 0.03 (r of 20 000 independent pairs has sigma 0.0071)."""
    x = B.bg_colour(5, np.arange(N_CALLS)).astype(np.float64)
    for c in range(3):
        m, v = x[:, c].mean(), x[:, c].var()
        print(f"component {c}: mean {m:.5f} variance {v:.5f} (1/12 = {1 / 12:.5f})")
        assert abs(m - 0.5) < 0.01 and abs(v - 1 / 12) < 0.005
    r = np.corrcoef(x.T)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        print(f"components {a},{b}: r = {r[a, b]:+.4f}")
        assert abs(r[a, b]) < 0.03
    for a in range(3):
        for b in range(3):
            rc = np.corrcoef(x[:-1, a], x[1:, b])[0, 1]
            print(f"call k component {a} vs call k+1 component {b}: r = {rc:+.4f}")
            assert abs(rc) < 0.03


def test_splitmix64_and_mix32_known_answers():
    """splitmix64(0) is the first output of the published SplitMix64 generator seeded with 0; mix32 is the
    low word of murmur3's fmix64, which maps 0 to 0."""
    assert int(B.splitmix64(0)) == 0xE220A8397B1DCDAF
    assert int(B.splitmix64(int(B.GOLDEN))) == 0x6E789E6AA1B965F4  # the generator's second output
    assert int(B.mix32(0)) == 0 and B.mix32(1).dtype == np.uint32
    assert int(B.mix32(1)) == 0xB456BCFC34C2CB2C & 0xFFFFFFFF       # fmix64(1)


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_header_and_ctypes_signature_agree(name):
    from mfnerf import _lib
    args = _declared_args(name)
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert len(args) == len(argtypes), (args, argtypes)
    scalars = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    for a, t in zip(args, argtypes):
        declared_ptr = "*" in a or a.startswith("mfnerf_stream_t")
        assert declared_ptr == (t is ctypes.c_void_p), (name, a, t)
        if not declared_ptr:
            assert t is scalars[a.split()[0]], (name, a, t)
    # the _bg forms differ from their scalar forms by the colour argument alone
    if name != "mfnerf_sample_rays_prep_bg":
        base = _declared_args(name[:-3])
        i = base.index("float bg_r")
        assert base[i:i + 3] == ["float bg_r", "float bg_g", "float bg_b"]
        assert args == base[:i] + ["const float* bg"] + base[i + 3:]
    else:
        base = _declared_args("mfnerf_sample_rays_prep_idx")
        assert args == base[:-1] + ["float* bg"] + base[-1:]


def test_library_exports_the_new_entry_points():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_null_bg_is_invalid_before_any_launch():
    """A null bg is MFN_ERR_INVALID, reported before anything touches the device (n_rays > 0, every
    other pointer null as well: the check comes first or the null-pointer check catches it)."""
    from mfnerf import _lib
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    assert lib.mfnerf_composite_train_fused_bg(z, z, z, z, z, 4, 16, 1e-4, z, 4, 1e-3, z, z, z, z, z, z, z, z, z, z, z,
                                               z) != 0
    assert b"bg" in lib.mfnerf_last_error()
    assert lib.mfnerf_nerf_loss_bg(z, z, z, 4, 4, 1e-3, z, z, z, z, z) != 0
    assert b"bg" in lib.mfnerf_last_error()
    assert lib.mfnerf_sample_rays_prep_bg(z, z, z, 1, 1, 4, 0, 0, z, z, z, z, 0.01, z, z, z, z, z, z) != 0


def test_step_config_and_hparams_carry_the_option():
    from mfnerf.engine import StepConfig, TrainStep
    from mfnerf.trainer import HParams
    assert StepConfig(random_bg=True).random_bg and not StepConfig().random_bg
    assert HParams(random_bg=True).random_bg and not HParams().random_bg
    # in effect on real scenes only (the reference draws a colour only when exp_step_factor != 0)
    assert TrainStep._random_bg(_NoInit(StepConfig(random_bg=True, scale=1.0)))
    assert not TrainStep._random_bg(_NoInit(StepConfig(random_bg=True, scale=0.5)))
    assert not TrainStep._random_bg(_NoInit(StepConfig(scale=16.0)))


def test_bg_argument_validation():
    from mfnerf.data import DeviceDataset
    from mfnerf.engine import StepConfig, TrainStep
    import torch
    with pytest.raises(ValueError, match="random_bg=True"):
        TrainStep._check_bg(_NoInit(StepConfig()), (0, 0, 0))
    with pytest.raises(ValueError, match="attached dataset"):
        TrainStep._check_bg(_NoInit(StepConfig(random_bg=True, scale=1.0), dataset=object()), None, (0, 0, 0))
    TrainStep._check_bg(_NoInit(StepConfig()), None, None)                          # nothing given: no check
    TrainStep._check_bg(_NoInit(StepConfig(random_bg=True, scale=1.0)), (0, 0, 0))  # the supported form
    ds = DeviceDataset(torch.zeros(1, 4, 3), torch.zeros(1, 3, 4), torch.zeros(4, 3), device="cpu")
    with pytest.raises(ValueError, match="prep="):
        ds.sample(torch.zeros(3, 8, 3), bg=torch.zeros(3))
