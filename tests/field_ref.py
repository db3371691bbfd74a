"""The NGP field head (csrc/field_fw.hip, field_bw.hip: xyz MLP 32->64->16, SH4, rgb MLP 32->W->W->3, TruncExp)
restated in plain torch with float64 accumulation, from the same fp16 points as the kernels.

oracle/field_oracle.py's ngp_field_fw16 / ngp_field_bw16 round every operand to fp16 where tcnn and the
kernels hold it in fp16 and accumulate in fp32, in torch's order.  Here the rounding points are the
same (weights, ReLU outputs, h, SH, and every data gradient after its ReLU mask) and every matrix
product and every sum over samples is taken in float64, so the result does not depend on a summation
order: it is what a kernel's fp32 MFMA sums are an approximation of.

    forward(feat16, dirs, px, pr, width)  -> sigma (N), rgb (N,3), acts
    backward(acts, dL_dsigma, dL_drgb, S) -> dL_dfeat (N,32), d xyz-MLP (3072), d rgb-MLP, unscaled
    take(acts, idx)                       -> the activations of the samples idx (weights kept)

A sample's rows depend on no other sample, so the reference of a launch that tiles a base block
(tile_rows) is the base block's reference gathered, and a weight gradient restricted to a region of
a launch is backward(take(acts, region's base rows), ...).

Where an fp16 rounding (or a ReLU gate) of the emulation falls the other way under fp32 and under
float64 accumulation, the emulation is deciding that rounding by its summation order, and a kernel
with a third order may land on either side: order_sensitivity measures it, and every input the GPU
tests use must keep it below ORDER_LIMIT (tests/test_field_ref_cpu.py asserts that on the CPU).

This module also owns the inputs of tests/test_gpu_field_seams.py (seam_inputs, the seeds, the region
tables), so that the CPU test checks exactly what the GPU file runs.
"""
import torch

from oracle import field_oracle as FO

F64 = torch.float64
ORDER_LIMIT = 2e-4   # test_field_bw_inputs' bound on its own order-sensitivity condition
S = 16384.0          # the loss scale of test_field_bw
BASE_N = 4999        # the base block every large launch tiles (prime: every sample recurs at other
                     # lane, wave, workgroup and pass positions)
SMALL_NS = (1, 31, 32, 33, 173)
# Seeds from a search on the CPU (running this file prints the table for seeds 1..39).  Over those
# seeds the worst sensitivity of a width's cases is either 1e-4..4e-4 (single fp16 roundings) or
# above 2e-3 (a ReLU gate flipped: 5 of 39 seeds at width 64, 15 of 39 at width 128, seed 1 at both).
# Chosen: the seeds with the lowest worst case, small N 5.3e-5 | 7.6e-5, base block and regions
# 1.14e-4 | 1.19e-4 (width 64 | 128).
SMALL_SEED = {64: 6, 128: 34}
BASE_SEED = {64: 6, 128: 34}


def rgb_net_params(width=64):
    return width * 32 + width * width + 16 * width


def _h(t):
    return t.half().to(F64)


def seam_inputs(n, seed, width):
    """test_gpu_field's _field_inputs at the Xavier scale plus test_field_bw's incoming gradients:
    feat f16 (n,32), dirs (n,3), px (3072), pr, dL_dsigma (n), dL_drgb (n,3), all on the CPU."""
    g = torch.Generator().manual_seed(seed)
    feat = (torch.rand(n, 32, generator=g) - 0.5).half()
    dirs = torch.randn(n, 3, generator=g)
    px = FO.xavier_uniform_(torch.empty(3072), FO.mlp_shapes(32, 16, 64, 1), g)
    pr = FO.xavier_uniform_(torch.empty(rgb_net_params(width)), FO.mlp_shapes(32, 3, width, 2), g)
    dsig = torch.randn(n, generator=g) * 1e-6
    drgb = torch.randn(n, 3, generator=g) * 1e-5
    return feat, dirs, px, pr, dsig, drgb


def tile_rows(n, base_n=BASE_N):
    """Base row of each of a launch's n samples: sample i is base sample i mod base_n."""
    return torch.arange(n) % base_n


def forward(feat16, dirs, px, pr, width=64):
    """ngp_field_fw16 with float64 products.  Returns sigma (N), rgb (N,3) and the activations."""
    W = width
    f = feat16.to(F64)
    W1 = _h(px[:2048].view(64, 32)); W2 = _h(px[2048:3072].view(16, 64))
    R1 = _h(pr[:W * 32].view(W, 32)); R2 = _h(pr[W * 32:W * 32 + W * W].view(W, W))
    R3 = _h(pr[W * 32 + W * W:].view(16, W))
    y1 = _h(torch.relu(f @ W1.t()))
    h = _h(y1 @ W2.t())
    dn = dirs / torch.norm(dirs, dim=1, keepdim=True)
    sh = _h(FO.sh4((dn + 1) / 2))  # the polynomial itself in fp32, as the oracle and the kernels
    inp = torch.cat([sh, h], 1)
    r1 = _h(torch.relu(inp @ R1.t()))
    r2 = _h(torch.relu(r1 @ R2.t()))
    rgb = torch.sigmoid((r2 @ R3.t())[:, :3])
    acts = dict(f=f, W1=W1, W2=W2, R1=R1, R2=R2, R3=R3, y1=y1, h=h, inp=inp, r1=r1, r2=r2, rgb=rgb)
    return torch.exp(h[:, 0]), rgb, acts


PER_SAMPLE = ("f", "y1", "h", "inp", "r1", "r2", "rgb")


def take(acts, idx):
    """The activations (of forward or of FO.ngp_field_fw16) of the samples idx; the weights kept."""
    return {k: (v[idx] if k in PER_SAMPLE else v) for k, v in acts.items()}


def backward(acts, dL_dsigma, dL_drgb, S=S):
    """ngp_field_bw16 with float64 products and sums over samples (the same fp16 rounding of every
    data gradient after its ReLU mask).  Returns dL_dfeat (N,32), the xyz weight gradient (3072:
    dW1, dW2) and the rgb weight gradient (dWr1, dWr2, dWr3), unscaled, float64."""
    a = acts
    N = a["f"].shape[0]
    rgb = a["rgb"].to(F64)
    dO = torch.zeros(N, 16, dtype=F64)
    dO[:, :3] = dL_drgb.to(F64) * S * rgb * (1 - rgb)
    dO = _h(dO)
    dWr3 = dO.t() @ a["r2"]
    dr2 = _h((dO @ a["R3"]) * (a["r2"] > 0))
    dWr2 = dr2.t() @ a["r1"]
    dr1 = _h((dr2 @ a["R2"]) * (a["r1"] > 0))
    dWr1 = dr1.t() @ a["inp"]
    dh = (dr1 @ a["R1"])[:, 16:].clone()
    dh[:, 0] += dL_dsigma.to(F64) * S * torch.exp(a["h"][:, 0].clamp(-15, 15))  # TruncExp backward
    dh = _h(dh)
    dW2 = dh.t() @ a["y1"]
    dy1 = _h((dh @ a["W2"]) * (a["y1"] > 0))
    dW1 = dy1.t() @ a["f"]
    dX = dy1 @ a["W1"]
    return (dX / S, torch.cat([dW1.flatten(), dW2.flatten()]) / S,
            torch.cat([dWr1.flatten(), dWr2.flatten(), dWr3.flatten()]) / S)


def level_l1_ref(dfeat):
    """What mfnerf_field_bw adds into level_l1 and mfnerf_grid_level_l1 computes: per level l of
    the 16, the sum over rows of |d[:, 2l]| + |d[:, 2l+1]|, float64."""
    d = dfeat.to(F64).abs()
    return d.view(d.shape[0], d.shape[1] // 2, 2).sum((0, 2))


def order_sensitivity(feat16, dirs, px, pr, dL_dsigma, dL_drgb, S=S, width=64, idx=None):
    """max|emulation (fp32 sums) - this reference| / max|this reference| for (dL_dfeat, gx, gr), over
    all samples or, with idx, over the samples idx alone (a region's weight gradients)."""
    _, _, a32 = FO.ngp_field_fw16(feat16, dirs, px, pr, width)
    _, _, a64 = forward(feat16, dirs, px, pr, width)
    return order_sensitivity_acts(a32, a64, dL_dsigma, dL_drgb, S, idx)


def order_sensitivity_acts(a32, a64, dL_dsigma, dL_drgb, S=S, idx=None):
    """order_sensitivity from the two forwards' activations (shared between a block's regions)."""
    if idx is not None:
        a32, a64, dL_dsigma, dL_drgb = take(a32, idx), take(a64, idx), dL_dsigma[idx], dL_drgb[idx]
    lo = FO.ngp_field_bw16(a32, dL_dsigma, dL_drgb, S)
    hi = backward(a64, dL_dsigma, dL_drgb, S)
    return tuple(float((l.to(F64) - w).abs().max() / w.abs().max()) for l, w in zip(lo, hi))


def fp32_autograd(feat, dirs, px, pr, dsig, drgb, width=64):
    """Plain fp32 autograd of the whole head (half-rounded weights, no other fp16 point):
    (dL_dfeat, d xyz-MLP, d rgb-MLP) of sum(sigma * dsig) + sum(rgb * drgb)."""
    f32 = feat.float().requires_grad_(True)
    a = px.half().float().requires_grad_(True)
    b = pr.half().float().requires_grad_(True)
    W = width
    W1 = a[:2048].view(64, 32); W2 = a[2048:3072].view(16, 64)
    R1 = b[:W * 32].view(W, 32); R2 = b[W * 32:W * 32 + W * W].view(W, W); R3 = b[W * 32 + W * W:].view(16, W)
    y1 = torch.relu(f32 @ W1.t()); h = y1 @ W2.t()
    sigma = torch.exp(h[:, 0])
    dn = dirs / torch.norm(dirs, dim=1, keepdim=True)
    r1 = torch.relu(torch.cat([FO.sh4((dn + 1) / 2), h], 1) @ R1.t()); r2 = torch.relu(r1 @ R2.t())
    c = torch.sigmoid(r2 @ R3.t())[:, :3]
    ((sigma * dsig).sum() + (c * drgb).sum()).backward()
    return f32.grad, a.grad, b.grad


# ---- the launches and spotlight regions of tests/test_gpu_field_seams.py
#
# G = mfnerf_field_bw_slab_rows(width) persistent workgroups take 128-sample groups g, g + G, ...; a
# launch of n samples is tile_rows(n) of the base block.  A region is a range [lo, hi) of a launch's
# samples: the incoming gradients are zero outside it, so the weight gradients are the region's own.


def launch_sizes(G, width):
    """name -> n of the backward launches."""
    out = {"two_pass": G * 128 + 173, "exact": G * 128, "exact_plus_1": G * 128 + 1}
    if width == 128:
        out["three_pass"] = 2 * G * 128 + 173
    return out


def regions(G, width):
    """(name, launch, lo, hi, slice_from): the spotlight regions; slice_from is the multiple of 128
    at or below lo from which the region's samples are launched on their own."""
    n2 = G * 128 + 173
    out = [("second_pass", "two_pass", G * 128, n2, G * 128),
           ("ragged_tile", "two_pass", (n2 - 1) // 32 * 32, n2, G * 128),
           ("pass_boundary", "two_pass", (G - 1) * 128, (G + 1) * 128, (G - 1) * 128),
           ("last_group", "exact", (G - 1) * 128, G * 128, (G - 1) * 128),
           ("last_group_p1", "exact_plus_1", (G - 1) * 128, G * 128, (G - 1) * 128),
           ("single_sample", "exact_plus_1", G * 128, G * 128 + 1, G * 128)]
    if width == 128:
        out.append(("third_pass", "three_pass", 2 * G * 128, 2 * G * 128 + 173, 2 * G * 128))
    return out


def base_block(width):
    """The base block's inputs and both forwards, computed once per width."""
    if width not in _base_cache:
        inp = seam_inputs(BASE_N, BASE_SEED[width], width)
        feat, dirs, px, pr = inp[:4]
        _, _, a32 = FO.ngp_field_fw16(feat, dirs, px, pr, width)
        sig, rgb, a64 = forward(feat, dirs, px, pr, width)
        _base_cache[width] = dict(inputs=inp, a32=a32, a64=a64, sigma=sig, rgb=rgb)
    return _base_cache[width]


_base_cache = {}


def worst_sensitivities(G, width, small_seed, base_seed):
    """Every precondition of the GPU file at these seeds: {case: (dfeat, gx, gr) sensitivities}."""
    out = {}
    for n in SMALL_NS:
        out[f"small_{n}"] = order_sensitivity(*seam_inputs(n, small_seed, width), S, width)
    feat, dirs, px, pr, dsig, drgb = seam_inputs(BASE_N, base_seed, width)
    _, _, a32 = FO.ngp_field_fw16(feat, dirs, px, pr, width)
    _, _, a64 = forward(feat, dirs, px, pr, width)
    out["base_block"] = order_sensitivity_acts(a32, a64, dsig, drgb, S)
    for name, _, lo, hi, _ in regions(G, width):
        out[name] = order_sensitivity_acts(a32, a64, dsig, drgb, S, torch.arange(lo, hi) % BASE_N)
    return out


if __name__ == "__main__":  # the seed search: python tests/field_ref.py
    from mfnerf._lib import load
    G_OF = {w: load().mfnerf_field_bw_slab_rows(w) for w in (64, 128)}
    for width in (64, 128):
        for seed in range(1, 40):
            w = worst_sensitivities(G_OF[width], width, seed, seed)
            small = max(max(v) for k, v in w.items() if k.startswith("small_"))
            big = max(max(v) for k, v in w.items() if not k.startswith("small_"))
            print(f"width {width} seed {seed}: small N worst {small:.2e}, base block and regions worst {big:.2e}")
