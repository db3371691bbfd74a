"""The standalone FullyFusedMLP (csrc/mlp.hip: 32 -> W [-> W] -> 16, bias-free, ReLU hidden layers,
output activation None or Sigmoid) restated in plain torch with float64 accumulation, from the same
fp16 points as the kernels.

The kernels hold weights, layer inputs and every data gradient in fp16 and accumulate in fp32 on
the MFMA unit, in an order of their own.  Here the rounding points are the same and every matrix
product and every sum over samples is taken in float64, so the result does not depend on a summation
order: it is what the kernels' fp32 sums are an approximation of.

    forward(x16, params, W, NH, OA)  -> y (N, 16) unrounded, acts
        weights -> fp16; a_0 = x16; a_{l+1} = fp16(relu(a_l W_l^T)); z = a_NH W_out^T (unrounded);
        y = z or sigmoid(z).  The kernel rounds y to fp16 when it stores it; compare with y.half().
    backward(acts, dout)             -> dx (N, 32), [dW_0 .. dW_NH]
        dZ_out = fp16(dout * y (1 - y)) with the unrounded y (None: fp16(dout)); dW_out = dZ_out^T a_NH;
        dZ_l = fp16((dZ_{l+1} W_{l+1}) * (a_{l+1} > 0)); dW_l = dZ_l^T a_l; dx = dZ_0 W_0 (unrounded:
        the kernel stores it as fp32).  dout is the (N, 16) fp16 buffer the C ABI takes.
    take(acts, idx)                  -> the activations of the samples idx (weights kept)

A sample's rows depend on no other sample, so the reference of a launch that tiles a base block
(tile_rows) is the base block's reference gathered, and a weight gradient restricted to a region of a
launch is backward(take(acts, region's base rows), dout[region's base rows]).

Where an fp16 rounding (or a ReLU gate) falls the other way under fp32 and under float64
accumulation, the restatement is deciding that rounding by its summation order, and a kernel with a
third order may land on either side: order_sensitivity measures it (the same restatement with
float32 products against this one), and every input the GPU tests use must keep it below
field_ref.ORDER_LIMIT (tests/test_mlp_ref_cpu.py asserts that on the CPU).  forward_sensitivity is the
same for the forward's fp16 outputs; it matters only where W_out is scaled up (the saturation inputs).

This module also owns the inputs of tests/test_gpu_mlp_seams.py (seam_inputs, the seeds, the launch
and region tables), so that the CPU test checks exactly what the GPU file runs.
"""
import torch

from mfnerf import tcnn as T

F64 = torch.float64
F32 = torch.float32
N_IN, N_OUT = 32, 16  # mlp.hip:28  constexpr int N_IN = 32, N_OUT = 16
TILE = 32             # mlp.hip:152 and :192  s = tile * 32 + (lane & 31): one wave, one 32-sample tile
WG = 128              # mlp.hip:151 and :191  tile = blockIdx.x * 4 + wid: 4 waves = 128 samples a workgroup
CH = 1024             # mlp.hip:263  constexpr int DW_CH = 1024: samples per split-K chunk of the dW GEMMs
TRIP = 4096 * 128     # mlp.hip:370 and :409  blocks = want < 4096 ? want : 4096: samples per grid trip
BASE_N = 4999         # the base block every launch above 173 samples tiles (prime: every sample recurs
                      # at other lane, wave, workgroup, chunk and trip positions)
SMALL_NS = (1, 31, 32, 33, 127, 129, 173)
CHUNK_NS = (1023, 1024, 1025, 2049)
SAT_N = 4000

CONFIGS = tuple((W, NH, OA) for W in (64, 128) for NH in (1, 2) for OA in ("None", "Sigmoid"))
# the backward's two-trip cases: tests/test_gpu_tcnn.py's first four CFGS and the HDR rgb_net at width 128
BW_TRIP_CONFIGS = ((64, 1, "None"), (64, 2, "Sigmoid"), (128, 2, "Sigmoid"), (128, 1, "None"), (128, 2, "None"))
SAT_CONFIGS = ((64, 2, "Sigmoid"), (128, 2, "Sigmoid"))

# Seeds from a search on the CPU (running this file prints the table).  SMALL_SEED covers SMALL_NS,
# BASE_SEED the base block, the chunk-seam prefixes, the single sample 1024 and every region.
# Over seeds 1..24 a config's worst case is 2e-5..3e-4 (single fp16 roundings) or, at width 128,
# above 1e-2 (a ReLU gate flipped: seeds 1, 15, 16, 23).  Chosen: the seed with the lowest worst case,
# 3.1e-5 .. 7.5e-5 per config.
_SEED = {(64, 1, "None"): 7, (64, 1, "Sigmoid"): 5, (64, 2, "None"): 3, (64, 2, "Sigmoid"): 16,
         (128, 1, "None"): 7, (128, 1, "Sigmoid"): 9, (128, 2, "None"): 2, (128, 2, "Sigmoid"): 7}
SMALL_SEED = dict(_SEED)
BASE_SEED = dict(_SEED)
# Saturation (W, 2, Sigmoid): (seed, scale of W_out).  A hidden activation whose fp16 rounding falls the
# other way moves a logit by ulp(a) * |W_out| * scale, so the scale that saturates the sigmoid also
# amplifies the summation order into the output (at scale 256 the float32 and float64 restatements
# differ by 2e-3..9e-3 in y) and, through y (1 - y), into dx (3e-4..3e-3).
#   "bounds":   the scale at which the forward and backward bounds mean something: at least 10 % of
#               the logits beyond +-15, order_sensitivity < ORDER_LIMIT and forward_sensitivity <=
#               FW_ORDER_LIMIT.  Of seeds 1..79 at scales 48..112: 33 % | 34 % of the logits beyond
#               +-15, forward 9.8e-4 | 7.3e-4, backward 7.6e-5 | 1.8e-4 (width 64 | 128).
#   "overflow": logits past -88.7, where exp(-z) is inf in fp32 (logits in [-97, 203] | [-105, 146],
#               75 % | 78 % beyond +-15): only what the summation order cannot move is compared there.
SAT = {"bounds": {64: (16, 64.0), 128: (13, 96.0)}, "overflow": {64: (9, 256.0), 128: (288, 256.0)}}
# The fp16 outputs of a sigmoid in [0.5, 1] lie on a grid of 2^-11 and the forward bound, 2e-3, is four
# steps of it: the two restatements may differ by two steps, which leaves the kernel the other two.
FW_ORDER_LIMIT = 2.0 ** -10


def n_out_of(NH, OA):
    """The live output columns of the inputs' dout: xyz_encoder's network feeds all 16 on, every
    other configuration is an rgb_net with 3."""
    return 16 if (OA == "None" and NH == 1) else 3


def shapes_of(W, NH):
    return T.mlp_shapes(N_IN, N_OUT, W, NH)


def n_params(W, NH):
    return sum(o * k for o, k in shapes_of(W, NH))


def seam_inputs(n, seed, W, NH, OA):
    """x f16 (n, 32) in [-0.5, 0.5), params at tcnn's Xavier scale, dout f16 (n, 16): tcnn's
    loss-scaled (x 128) incoming gradient in the live columns, zero in the padding.  On the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, N_IN, generator=g) - 0.5).half()
    params = T._xavier(shapes_of(W, NH), g)
    n_out = n_out_of(NH, OA)
    dout = torch.zeros(n, N_OUT, dtype=torch.float16)
    dout[:, :n_out] = (torch.randn(n, n_out, generator=g) * 1e-2 * 128).half()
    return x, params, dout


def saturation_inputs(W, case="bounds"):
    """The first SAT_N samples of a base block of (W, 2, Sigmoid) with W_out scaled: SAT[case][W]."""
    seed, scale = SAT[case][W]
    x, params, dout = seam_inputs(BASE_N, seed, W, 2, "Sigmoid")
    params = params.clone()
    params[n_params(W, 2) - N_OUT * W:] *= scale
    return x[:SAT_N].contiguous(), params, dout[:SAT_N].contiguous()


def tile_rows(n, base_n=BASE_N):
    """Base row of each of a launch's n samples: sample i is base sample i mod base_n."""
    return torch.arange(n) % base_n


def forward(x16, params, W, NH, OA, dtype=F64, rnd=None):
    """The forward with products in `dtype`.  rnd is the fp16 rounding (identity for the formula
    check against autograd).  Returns y (N, 16), unrounded, and the activations."""
    r = rnd or (lambda t: t.half().to(dtype))
    Ws, off = [], 0
    for o, k in shapes_of(W, NH):
        Ws.append(r(params[off:off + o * k].view(o, k).to(dtype)))
        off += o * k
    a = [x16.to(dtype)]
    for l in range(NH):
        a.append(r(torch.relu(a[-1] @ Ws[l].t())))
    z = a[-1] @ Ws[NH].t()
    y = torch.sigmoid(z) if OA == "Sigmoid" else z
    return y, dict(a=a, Ws=Ws, z=z, y=y, OA=OA)


def take(acts, idx):
    """The activations of the samples idx; the weights kept."""
    return dict(a=[t[idx] for t in acts["a"]], Ws=acts["Ws"], z=acts["z"][idx], y=acts["y"][idx], OA=acts["OA"])


def backward(acts, dout, rnd=None):
    """The backward from the (N, 16) dout, products and sums over samples in the activations' dtype.
    Returns dx (N, 32) and the list of the layers' dW, W_0 first."""
    a, Ws, y = acts["a"], acts["Ws"], acts["y"]
    dtype = y.dtype
    r = rnd or (lambda t: t.half().to(dtype))
    NH = len(Ws) - 1
    d = dout.to(dtype)
    if acts["OA"] == "Sigmoid":
        d = d * (y * (1 - y))
    dz = r(d)
    dWs = [None] * (NH + 1)
    dWs[NH] = dz.t() @ a[NH]
    for l in range(NH - 1, -1, -1):
        dz = r((dz @ Ws[l + 1]) * (a[l + 1] > 0))
        dWs[l] = dz.t() @ a[l]
    return dz @ Ws[0], dWs


def flat(dWs):
    """The layers' dW in the parameter layout of `grad`."""
    return torch.cat([w.flatten() for w in dWs])


def split(grad, W, NH):
    """A flat gradient as the list of the layers' dW."""
    out, off = [], 0
    for o, k in shapes_of(W, NH):
        out.append(grad[off:off + o * k].view(o, k))
        off += o * k
    return out


def order_sensitivity(x16, params, dout, W, NH, OA, idx=None):
    """max|float32 restatement - this reference| / max|this reference| for (dx, dW_0, .., dW_NH), over
    all samples or, with idx, over the samples idx alone (a region's weight gradients)."""
    _, a32 = forward(x16, params, W, NH, OA, F32)
    _, a64 = forward(x16, params, W, NH, OA)
    return order_sensitivity_acts(a32, a64, dout, idx)


def order_sensitivity_acts(a32, a64, dout, idx=None):
    """order_sensitivity from the two forwards' activations (shared between a block's regions)."""
    if idx is not None:
        a32, a64, dout = take(a32, idx), take(a64, idx), dout[idx]
    lo_x, lo_w = backward(a32, dout)
    hi_x, hi_w = backward(a64, dout)
    return tuple(float((l.to(F64) - h).abs().max() / h.abs().max()) for l, h in zip([lo_x] + lo_w, [hi_x] + hi_w))


# ---- the launches and spotlight regions of tests/test_gpu_mlp_seams.py
#
# mfnerf_mlp_fw / _bw launch min(ceil(n / 128), 4096) workgroups; workgroup b's wave w takes the tiles
# 4 b + w, 4 b + w + 4 * 4096, ...: the second trip starts at sample TRIP.  mlp_dw_kernel's workgroup
# k sums the samples [k CH, (k + 1) CH) of the padded length ld = ceil32(n).  A launch of n samples is
# tile_rows(n) of the base block.  A region is a range [lo, hi) of a launch's samples: dout is zero
# outside it, so the weight gradients are the region's own.


def launch_sizes():
    """name -> n of the launches."""
    return {"two_trip": TRIP + 173, "base": BASE_N, "exact": TRIP, "exact_plus_1": TRIP + 1}


def regions():
    """(name, launch, lo, hi, slice_from): the spotlight regions; slice_from is the multiple of CH
    at or below lo from which the region's samples are launched on their own."""
    n2 = TRIP + 173
    return [("second_trip", "two_trip", TRIP, n2, TRIP),
            ("ragged_tile", "two_trip", (n2 - 1) // TILE * TILE, n2, TRIP),
            ("trip_boundary", "two_trip", TRIP - 128, TRIP + 128, TRIP - CH),
            ("chunk_boundary", "base", 3 * CH - 32, 3 * CH + 32, 2 * CH),
            ("last_chunk", "exact", TRIP - CH, TRIP, TRIP - CH),
            ("single_sample", "exact_plus_1", TRIP, TRIP + 1, TRIP)]


def base_block(cfg):
    """The base block's inputs and both forwards, computed once per (W, NH, OA)."""
    if cfg not in _base_cache:
        x, params, dout = seam_inputs(BASE_N, BASE_SEED[cfg], *cfg)
        _, a32 = forward(x, params, *cfg, F32)
        y, a64 = forward(x, params, *cfg)
        _base_cache[cfg] = dict(inputs=(x, params, dout), a32=a32, a64=a64, y=y)
    return _base_cache[cfg]


_base_cache = {}


def forward_sensitivity(x16, params, W, NH, OA):
    """max|float32 restatement - this reference| over the forward's outputs, both rounded to fp16."""
    y32, _ = forward(x16, params, W, NH, OA, F32)
    y64, _ = forward(x16, params, W, NH, OA)
    return float((y32.half().to(F64) - y64.half().to(F64)).abs().max())


def saturation_stats(W, case="bounds"):
    """(share of the logits of the live columns beyond +-15, their minimum, their maximum) of the
    reference at saturation_inputs(W, case)."""
    x, params, dout = saturation_inputs(W, case)
    _, acts = forward(x, params, W, 2, "Sigmoid")
    z = acts["z"][:, :3]
    return float((z.abs() > 15).double().mean()), float(z.min()), float(z.max())


def worst_sensitivities(cfg, small_seed, base_seed):
    """Every precondition of the GPU file at these seeds: {case: (dx, dW_0, .., dW_NH) sensitivities}."""
    out = {}
    for n in SMALL_NS:
        out[f"small_{n}"] = order_sensitivity(*seam_inputs(n, small_seed, *cfg), *cfg)
    x, params, dout = seam_inputs(BASE_N, base_seed, *cfg)
    _, a32 = forward(x, params, *cfg, F32)
    _, a64 = forward(x, params, *cfg)
    out["base_block"] = order_sensitivity_acts(a32, a64, dout)
    for n in CHUNK_NS:
        out[f"chunk_{n}"] = order_sensitivity_acts(a32, a64, dout, torch.arange(n))
    out["sample_1024"] = order_sensitivity_acts(a32, a64, dout, torch.arange(1024, 1025))
    for name, _, lo, hi, _ in regions():
        out[name] = order_sensitivity_acts(a32, a64, dout, torch.arange(lo, hi) % BASE_N)
    return out


def saturation_sensitivity(W, case="bounds"):
    """(forward_sensitivity, order_sensitivity) of saturation_inputs(W, case)."""
    x, params, dout = saturation_inputs(W, case)
    return forward_sensitivity(x, params, W, 2, "Sigmoid"), order_sensitivity(x, params, dout, W, 2, "Sigmoid")


if __name__ == "__main__":  # the seed search: python tests/mlp_ref.py
    for cfg in CONFIGS:
        for seed in range(1, 25):
            w = worst_sensitivities(cfg, seed, seed)
            small = max(max(v) for k, v in w.items() if k.startswith("small_"))
            big = max(max(v) for k, v in w.items() if not k.startswith("small_"))
            print(f"{cfg} seed {seed}: small N worst {small:.2e}, base block, chunks and regions worst {big:.2e}",
                  flush=True)
    for W in (64, 128):
        for seed in range(1, 80):
            for scale in (48.0, 64.0, 80.0, 96.0, 112.0, 256.0):
                SAT["bounds"][W] = (seed, scale)
                share, lo, hi = saturation_stats(W)
                fw, bw = saturation_sensitivity(W)
                print(f"saturation W={W} seed {seed} scale {scale}: {share:.3f} beyond +-15, logits in "
                      f"[{lo:.1f}, {hi:.1f}], forward {fw:.2e}, backward worst {max(bw):.2e}", flush=True)
