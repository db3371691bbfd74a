"""Generate tests/golden/hdr_forward.npz by running the REFERENCE's own NGP(rgb_act='None').forward
and log_radiance_to_rgb (models/networks.py:111-155) on seeded inputs.

As make_golden.py, the reference is imported with its native dependencies replaced by restatements:
vren and the grid / SH / 32-wide networks by the CPU oracle (their outputs rounded to half, the
dtype tcnn returns), and tcnn.Network(1, 1, ...), the tonemapper, by the fp64 specification of
tests/tonemap_ref.py.  What this pins is the reference's HOST composition around the kernels:
(x - xyz_min) / (xyz_max - xyz_min), the SH input (d + 1) / 2, the concatenation order [d, h],
+ log(exposure), the channel order of the three tonemappers, and output_radiance.  Only data
(inputs, parameters, outputs) is written.

Run from anywhere:  python tests/golden/make_golden_hdr.py   (needs the reference tree, see
make_golden.py; CPU only)
"""
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import make_golden as MG  # noqa: E402
import tonemap_ref as R  # noqa: E402
from oracle import field_oracle  # noqa: E402

N_POINTS = 128
TABLE_SEED = 7


class HP:
    """The opt.py fields NGP reads, at the fixture's size (T = 2^14)."""
    grid, L, F, T, N_min, N_max, N_tables, rgb_channels, rgb_layers = "Hash", 16, 2, 14, 4, 256, 1, 64, 2


_seeds = itertools.count(100)


class Tonemapper(torch.nn.Module):
    """tcnn.Network(1, 1, ReLU/Sigmoid, 64 neurons, 1 hidden layer): the specification, fp64 out."""

    def __init__(self):
        super().__init__()
        self.params = torch.nn.Parameter(R.xavier_params(1, seed=next(_seeds)))

    def forward(self, x):  # x = log-radiance + log-exposure, added in fp32 by the reference
        return R.forward(x.float().half(), None, self.params)["y"]


class HalfNetwork(field_oracle.Network):
    def forward(self, x):
        return super().forward(x).half()


class HalfNetworkWithInputEncoding(field_oracle.NetworkWithInputEncoding):
    def forward(self, x):
        return super().forward(x).half()


def network(n_input_dims, n_output_dims, network_config, seed=1337):
    if n_input_dims == 1 and n_output_dims == 1:
        return Tonemapper()
    return HalfNetwork(n_input_dims, n_output_dims, network_config, seed=seed)


def main():
    MG.install_stubs()
    tc = sys.modules["tinycudann"]
    tc.Network, tc.NetworkWithInputEncoding = network, HalfNetworkWithInputEncoding
    import warnings
    warnings.filterwarnings("ignore")
    from models.networks import NGP

    model = NGP(scale=0.5, hparams=HP, rgb_act="None")
    n_net = model.xyz_encoder.n_net
    with torch.no_grad():  # a field that varies over the box (the fixture is about semantics)
        tab, g = MG.table_values(model.xyz_encoder.params.numel() - n_net, seed=TABLE_SEED)
        model.xyz_encoder.params[n_net:].copy_(tab)
        model.xyz_encoder.params[:n_net].mul_(2)
        model.rgb_net.params.mul_(2)
    x = torch.empty(N_POINTS, 3).uniform_(-0.5, 0.5, generator=g)
    d = torch.randn(N_POINTS, 3, generator=g) * torch.empty(N_POINTS, 1).uniform_(0.5, 2.0, generator=g)
    e = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (N_POINTS,), generator=g)].reshape(-1, 1)
    # the reference takes torch.log of the exposure; the fixture's values are ones whose fp32 log is
    # the correctly rounded one, as the specification has it
    assert torch.equal(torch.log(e), R.log_exposure(e, N_POINTS))
    with torch.no_grad():
        sigmas, rgbs = model(x, d, exposure=e)
        _, rgbs_unit = model(x, d)
        _, rgbs_scalar = model(x, d, exposure=torch.tensor(4.0))
        _, radiance = model(x, d, output_radiance=True)
        # the log-radiance the model fed its tonemappers (rgb_net's half output)
        xn = (x - model.xyz_min) / (model.xyz_max - model.xyz_min)
        h = model.xyz_encoder(xn)
        dn = d / torch.norm(d, dim=1, keepdim=True)
        lograd = model.rgb_net(torch.cat([model.dir_encoder((dn + 1) / 2), h], 1))
        # (outside autocast the reference's TruncExp runs in the half dtype of its input)
        assert torch.allclose(torch.exp(lograd.float()), radiance.float(), rtol=2.0 ** -10, atol=0)
        # train.py:172-177: zero log-radiance at unit exposure
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3), exposure=torch.ones(1, 1))
    out = {
        "x": x, "d": d, "exposure": e, "table_seed": torch.tensor(TABLE_SEED),
        "xyz_net_params": model.xyz_encoder.params[:n_net].detach(), "rgb_params": model.rgb_net.params.detach(),
        "tonemapper_params": torch.stack([getattr(model, f"tonemapper_net_{i}").params.detach() for i in range(3)]),
        "sigmas": sigmas.float(), "lograd": lograd, "radiance": radiance.float(), "rgb": rgbs, "rgb_unit": rgbs_unit,
        "rgb_scalar4": rgbs_scalar, "unit_exposure_rgb": unit,
    }
    np.savez_compressed(os.path.join(HERE, "hdr_forward.npz"), **{k: v.numpy() for k, v in out.items()})
    print("wrote hdr_forward.npz:", {k: (tuple(v.shape), str(v.dtype)) for k, v in out.items()})
    print("log-radiance range", float(lograd.min()), float(lograd.max()), "rgb range", float(rgbs.min()),
          float(rgbs.max()))


if __name__ == "__main__":
    main()
