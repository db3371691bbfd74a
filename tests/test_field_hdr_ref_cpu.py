"""tests/field_hdr_ref.py (the field head without its output sigmoid, float64) on the CPU:

1. its forward is field_ref.forward's up to the last layer, and the log-radiance is the logit of
   field_ref's rgb (to the half rounding of the log-radiance);
2. its backward agrees with field_ref.backward fed g * y (1 - y): the two differ only in where the
   product with y (1 - y) is rounded, so they part only where an fp16 rounding of dO flips;
3. order_sensitivity (field_ref's method) < field_ref.ORDER_LIMIT for every (N, seed, width, region)
   tests/test_gpu_field_hdr.py runs, dL/dSH of the small N included.
"""
import pytest
import torch

import field_hdr_ref as H
import field_ref as R

WIDTHS = (64, 128)


def _slab_rows(width):
    from mfnerf._lib import load
    return load().mfnerf_field_bw_slab_rows(width)


@pytest.fixture(scope="module", params=WIDTHS)
def block(request):
    width = request.param
    feat, dirs, px, pr, dsig, dlog = R.seam_inputs(173, H.SMALL_SEED[width], width)
    s, rgb, acts = R.forward(feat, dirs, px, pr, width)
    sh, lograd, acts_h = H.forward(feat, dirs, px, pr, width)
    return dict(width=width, s=s, rgb=rgb, acts=acts, sh=sh, lograd=lograd, acts_h=acts_h, dsig=dsig, dlog=dlog)


def test_forward_is_the_head_without_its_sigmoid(block):
    b = block
    assert torch.equal(b["sh"], b["s"]), "sigma: the code is shared up to the epilogue"
    assert b["lograd"].shape == (173, 3) and b["lograd"].dtype == torch.float64
    assert torch.equal(b["lograd"], b["lograd"].half().double()), "log-radiance is tcnn's fp16 output"
    logit = torch.log(b["rgb"] / (1 - b["rgb"]))
    # half rounding: relative 2^-11, the subnormal step below 2^-14
    assert bool(((b["lograd"] - logit).abs() <= 2.0 ** -11 * logit.abs() + 2.0 ** -25).all())


def test_backward_is_field_ref_with_dO_of_g_times_S(block):
    """The restatement written out: dO = half(g * S), then field_ref.backward's chain."""
    b = block
    a, S = b["acts"], R.S
    dO = torch.zeros(173, 16, dtype=torch.float64)
    dO[:, :3] = b["dlog"].double() * S
    dO = dO.half().double()
    got = H.backward(a, b["dsig"], b["dlog"])
    assert torch.equal(got[2][-16 * b["width"]:].view(16, -1), (dO.t() @ a["r2"]) / S)
    dr2 = ((dO @ a["R3"]) * (a["r2"] > 0)).half().double()
    dr1 = ((dr2 @ a["R2"]) * (a["r1"] > 0)).half().double()
    assert torch.equal(H.dsh(a, b["dlog"]), (dr1 @ a["R1"])[:, :16] / S)


def test_backward_agrees_with_the_sigmoid_backward_fed_g_y_1_minus_y(block):
    b = block
    y = b["rgb"]
    eff = b["dlog"].double() * y * (1 - y)          # what the sigmoid would hand down
    want = H.backward(b["acts"], b["dsig"], eff)
    got = R.backward(b["acts"], b["dsig"], b["dlog"])  # field_ref: dO = half(g * S * y * (1 - y))
    for name, g, w in zip(("dL_dfeat", "gx", "gr"), got, want):
        err = float((g - w).abs().max() / w.abs().max())
        print(f"W={b['width']} {name}: {err:.3e}")
        # the same float64 product in another order (1e-16): they part only at a flipped fp16
        # rounding of dO, one half-ulp (2^-11) of one sample's term
        assert err < 2.0 ** -11, (name, err)


@pytest.mark.parametrize("width", WIDTHS)
def test_order_sensitivity_of_every_gpu_input(width):
    G = _slab_rows(width)
    worst = H.worst_sensitivities(G, width, H.SMALL_SEED[width], H.BASE_SEED[width])
    expected = {f"{k}_{n}" for n in R.SMALL_NS for k in ("small", "dsh")} | {"base_block"} | set(H.REGIONS)
    assert set(worst) == expected
    for case, sens in worst.items():
        print(f"W={width} {case}: order sensitivity " + " ".join(f"{s:.2e}" for s in sens))
    for case, sens in worst.items():
        assert max(sens) < R.ORDER_LIMIT, (width, case, sens)


def test_order_sensitivity_sees_a_bad_seed():
    """Not vacuous: seed 1 at width 64 flips a ReLU gate in the base block (the seed search: 2.9e-2)."""
    feat, dirs, px, pr, dsig, dlog = R.seam_inputs(R.BASE_N, 1, 64)
    from oracle import field_oracle as FO
    _, _, a32 = FO.ngp_field_fw16(feat, dirs, px, pr, 64)
    _, _, a64 = H.forward(feat, dirs, px, pr, 64)
    assert max(H.order_sensitivity_acts(a32, a64, dsig, dlog)) > 10 * R.ORDER_LIMIT
