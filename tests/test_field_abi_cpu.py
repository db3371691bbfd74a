"""The field head's C entry points (every mfnerf_field_* and mfnerf_sh4_fw) without a GPU: their
argument checks come before any HIP call, so a refused call touches no device.  Status codes and
error texts are asserted verbatim: they are part of the ABI the Python wrappers report."""
import ctypes

import pytest

OK, INVALID = 0, 1
BAD_WIDTH = "field: rgb_width=32 unsupported (this build: 64 or 128)"
BW_BAD = "field_bw: bad size, plane stride or grad_scale (0 = dynamic needs amp)"

# argument names in ABI order; a name in REQUIRED must be non-null once n > 0
FW = {
    "mfnerf_field_fw": ("feat ps dirs n n_dev packed width density_only sigma rgb stream", "field_fw",
                        "feat packed sigma dirs rgb"),
    "mfnerf_field_fw_lograd": ("feat ps dirs n n_dev packed width sigma lograd stream", "field_fw_lograd",
                               "feat packed sigma dirs lograd"),
    "mfnerf_field_fw_density_scatter": ("feat ps n n_dev packed width sigma cell_idx tmp stream",
                                        "field_fw_density_scatter", "feat packed sigma cell_idx tmp"),
}
_BW_ARGS = "feat ps dirs n n_dev packed width dL_dsigma dL_drgb grad_scale dL_dfeat grad_xyz grad_rgb workspace amp level_l1"
_BW_REQ = "feat dirs packed dL_dsigma dL_drgb dL_dfeat workspace"
BW = {
    "mfnerf_field_bw": (_BW_ARGS + " stream", _BW_REQ),
    "mfnerf_field_bw_lograd": (_BW_ARGS + " stream", _BW_REQ),
    "mfnerf_field_bw_inputs": (_BW_ARGS + " dL_ddirs stream", _BW_REQ + " dL_ddirs"),
    "mfnerf_field_bw_inputs_lograd": (_BW_ARGS + " dL_ddirs stream", _BW_REQ + " dL_ddirs"),
}
SCALARS = {"ps": 0, "n": 8, "width": 64, "density_only": 0, "grad_scale": 1.0}
OPTIONAL = ("n_dev", "stream", "amp", "level_l1")


@pytest.fixture(scope="module")
def lib():
    from mfnerf import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    """A non-null pointer that no refused call dereferences."""
    mem = ctypes.create_string_buffer(64)
    return mem, ctypes.c_void_p(ctypes.addressof(mem))


def _call(lib, name, names, some, **over):
    """Call `name` with every pointer non-null (optional ones null) and valid scalars, except `over`."""
    null = ctypes.c_void_p(0)
    args = []
    for a in names.split():
        if a in over:
            v = over[a]
            args.append(null if v is None else v)
        elif a in SCALARS:
            args.append(SCALARS[a])
        else:
            args.append(null if a in OPTIONAL else some)
    return getattr(lib, name)(*args)


def _refused(lib, status, text):
    assert status == INVALID
    assert lib.mfnerf_last_error().decode() == text


def _all_null(names):
    return {a: None for a in names.split() if a not in SCALARS}


@pytest.mark.parametrize("name", sorted(FW))
def test_forward_entry_points_refuse_before_the_device(lib, buf, name):
    names, prefix, required = FW[name]
    some = buf[1]
    _refused(lib, _call(lib, name, names, some, width=32), BAD_WIDTH)
    _refused(lib, _call(lib, name, names, some, n=-1), prefix + ": bad size")
    _refused(lib, _call(lib, name, names, some, n=8, ps=7), prefix + ": bad size")
    for a in required.split():
        _refused(lib, _call(lib, name, names, some, **{a: None}), prefix + ": null pointer")
    if "density_only" in names.split():  # the density-only form still needs its own three
        for a in ("feat", "packed", "sigma"):
            _refused(lib, _call(lib, name, names, some, density_only=1, **{a: None}), prefix + ": null pointer")
    assert _call(lib, name, names, some, n=0, **_all_null(names)) == OK
    # the width is checked first, the sizes before the pointers
    _refused(lib, _call(lib, name, names, some, width=32, n=-1, **_all_null(names)), BAD_WIDTH)
    _refused(lib, _call(lib, name, names, some, n=-1, **_all_null(names)), prefix + ": bad size")


@pytest.mark.parametrize("name", sorted(BW))
def test_backward_entry_points_refuse_before_the_device(lib, buf, name):
    names, required = BW[name]
    some = buf[1]
    _refused(lib, _call(lib, name, names, some, width=32), BAD_WIDTH)
    _refused(lib, _call(lib, name, names, some, n=-1), BW_BAD)
    _refused(lib, _call(lib, name, names, some, n=8, ps=7), BW_BAD)
    _refused(lib, _call(lib, name, names, some, grad_scale=0.0), BW_BAD)  # dynamic scale without amp
    _refused(lib, _call(lib, name, names, some, grad_scale=-1.0), BW_BAD)
    _refused(lib, _call(lib, name, names, some, grad_scale=float("nan")), BW_BAD)
    for a in required.split():
        _refused(lib, _call(lib, name, names, some, **{a: None}), "field_bw: null pointer")
    # grad_xyz and grad_rgb: both (fold now) or neither (deferred fold)
    _refused(lib, _call(lib, name, names, some, grad_xyz=None), "field_bw: null pointer")
    _refused(lib, _call(lib, name, names, some, grad_rgb=None), "field_bw: null pointer")
    assert _call(lib, name, names, some, n=0, **_all_null(names)) == OK
    _refused(lib, _call(lib, name, names, some, n=0, grad_scale=0.0, **_all_null(names)), BW_BAD)
    _refused(lib, _call(lib, name, names, some, width=32, n=-1, **_all_null(names)), BAD_WIDTH)


@pytest.mark.parametrize("name", ["mfnerf_field_bw_reduce", "mfnerf_field_bw_reduce_store"])
def test_slab_fold_entry_points_refuse_before_the_device(lib, buf, name):
    names = "width workspace grad_xyz grad_rgb nonfinite stream"
    some = buf[1]
    _refused(lib, _call(lib, name, names, some, width=32), BAD_WIDTH)
    for a in ("workspace", "grad_xyz", "grad_rgb"):
        _refused(lib, _call(lib, name, names, some, **{a: None}), "field_bw_reduce: null pointer")


@pytest.mark.parametrize("name", ["mfnerf_field_pack_weights", "mfnerf_field_pack_weights_f16"])
def test_pack_entry_points_refuse_before_the_device(lib, buf, name):
    names = "params_xyz params_rgb width packed stream"
    some = buf[1]
    _refused(lib, _call(lib, name, names, some, width=32), BAD_WIDTH)
    for a in ("params_xyz", "params_rgb", "packed"):
        _refused(lib, _call(lib, name, names, some, **{a: None}), name[len("mfnerf_"):] + ": null pointer")


def test_sh4_fw_refuses_before_the_device(lib, buf):
    names = "dirs01 n out stream"
    some = buf[1]
    _refused(lib, _call(lib, "mfnerf_sh4_fw", names, some, n=-1), "sh4_fw: bad arguments")
    _refused(lib, _call(lib, "mfnerf_sh4_fw", names, some, dirs01=None), "sh4_fw: bad arguments")
    _refused(lib, _call(lib, "mfnerf_sh4_fw", names, some, out=None), "sh4_fw: bad arguments")
    assert _call(lib, "mfnerf_sh4_fw", names, some, n=0, dirs01=None, out=None) == OK


def test_size_queries(lib):
    """44 | 106 fragments of 1 KiB; 512 | 256 slab rows of 3072 + (32 W + W^2 + 16 W) floats."""
    for w in (0, 32, 96, 256, -64):
        assert lib.mfnerf_field_packed_bytes(w) == -1
        assert lib.mfnerf_field_bw_slab_rows(w) == -1
        assert lib.mfnerf_field_bw_workspace(1000, w) == -1
    assert lib.mfnerf_field_packed_bytes(64) == 44 * 1024
    assert lib.mfnerf_field_packed_bytes(128) == 106 * 1024
    assert lib.mfnerf_field_bw_slab_rows(64) == 512
    assert lib.mfnerf_field_bw_slab_rows(128) == 256
    for n in (0, 1000, 1 << 20):  # the slab does not depend on n
        assert lib.mfnerf_field_bw_workspace(n, 64) == 512 * 10240 * 4
        assert lib.mfnerf_field_bw_workspace(n, 128) == 256 * 25600 * 4
