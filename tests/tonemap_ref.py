"""The specification of the HDR tonemappers (mfnerf.tonemap, csrc/tonemap.hip; INTEGRATION.md
"Tonemapper semantics") in fp64, from the same fp16 points as the kernels.

One tonemapper is tcnn.Network(1, 1, FullyFusedMLP ReLU/Sigmoid, 64 neurons, 1 hidden layer): 2048
fp32 parameters, W1 (64,16) row-major then W2 (16,64) row-major, the scalar input padded to the row
[x, 1, ..., 1].  With the weights rounded to half (W1h, W2h) and b_j = sum_{k=1..15} W1h[j,k]:

    x16 = half(float(lograd) + log e)          log e rounded to fp32, 0 without an exposure
    h_j = half(relu(W1h[j,0] * x16 + b_j))
    y   = sigmoid(sum_j W2h[0,j] * h_j)        (the kernel stores half(y))

    dz = dy * y * (1 - y)                      y = the saved (half) output
    dh_j = dz * W2h[0,j] where h_j > 0
    dlograd = sum_j dh_j * W1h[j,0]
    dW1[j,0] = sum_s dh_j * x16,  dW1[j,k>=1] = sum_s dh_j,  dW2[0,j] = sum_s dz * h_j,  dW2[1..15] = 0

Beside every value the functions return the sum of the absolute values of the terms they added, which
is what a rounding-error bound of the fp32 kernels scales with.
"""
import numpy as np
import torch

N_PARAMS = 2048
KINK = 1e-5  # |pre-activation| below this: the ReLU gate may fall either way in fp32


def xavier_params(C, seed=0):
    """C tonemappers' parameters (C * 2048) f32: Xavier-uniform per layer like tcnn, from a seeded
    CPU generator."""
    g = torch.Generator().manual_seed(seed)
    s = (6.0 / (64 + 16)) ** 0.5
    return torch.empty(C * N_PARAMS).uniform_(-s, s, generator=g)


EXPOSURES = ("none", "scalar_1_60", "scalar_32", "per_sample")


def make_inputs(n, C, exposure, seed=0):
    """The kernel tests' inputs: log-radiance U(-6,6) rounded to half (n,C), the exposure (None, a 0-d
    tensor, or n values drawn from {0.25, 1, 4}) and seed-0 Xavier parameters, all on the CPU.
    (The log-radiance generator's seed is the first one at which the specification flags no sample of
    the sizes below 100 as sitting on a ReLU kink: the tests' 1 % cap allows none there, and a draw of
    63 samples meets one about once in ten; test_tonemap_cpu.py checks the cap for every case.)"""
    g = torch.Generator().manual_seed(seed + 3)
    lograd = torch.empty(n, C).uniform_(-6, 6, generator=g).half()
    e = {"none": None, "scalar_1_60": torch.tensor(1 / 60), "scalar_32": torch.tensor(32.0),
         "per_sample": torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n,), generator=g)]}[exposure]
    return lograd, e, xavier_params(C, seed)


def weights(params, C):
    """(W1h (C,64,16), W2h (C,16,64)) fp64 values of the half-rounded parameters."""
    p = params.detach().cpu().float().reshape(C, N_PARAMS).half().double()
    return p[:, :1024].reshape(C, 64, 16), p[:, 1024:].reshape(C, 16, 64)


def log_exposure(exposure, n):
    """(n, 1) f32 log-exposure: the natural log in fp64, rounded to fp32; None -> 0."""
    if exposure is None:
        return torch.zeros(n, 1, dtype=torch.float32)
    e = torch.as_tensor(exposure).detach().cpu().float().reshape(-1)
    le = torch.from_numpy(np.log(e.double().numpy())).float()
    return le.expand(n).reshape(n, 1) if le.numel() == 1 else le.reshape(n, 1)


def points(lograd16, exposure):
    """x16 (n, C) as fp64: half(float(lograd) + log e), the addition in fp32."""
    l = lograd16.detach().cpu().half().float()
    return (l + log_exposure(exposure, l.shape[0])).half().double()


def forward(lograd16, exposure, params):
    """-> dict: y (n,C) fp64 (unrounded sigmoid), B (n,C) = sum_j |W2h[0,j] h_j|, kink (n) bool,
    x16 (n,C), h (n,C,64) (half-rounded), pre (n,C,64)."""
    C = lograd16.shape[1]
    W1, W2 = weights(params, C)
    x = points(lograd16, exposure)
    b = W1[:, :, 1:].sum(-1)                                    # (C,64)
    pre = x[:, :, None] * W1[None, :, :, 0] + b[None]           # (n,C,64)
    h = pre.clamp(min=0).half().double()
    t = h * W2[None, :, 0, :]
    return {"y": torch.sigmoid(t.sum(-1)), "B": t.abs().sum(-1), "kink": (pre.abs() < KINK).any(-1).any(-1),
            "x16": x, "h": h, "pre": pre}


def backward(lograd16, exposure, params, y_saved, dy, keep=None):
    """The gradients for the upstream dy (n,C), with y_saved (n,C) in place of the forward's own
    output; keep (n) bool = the samples that count towards the parameter gradient (default all).
    -> dict: dx (n,C), A_s (n,C); g (C*2048), A (C*2048)."""
    C = lograd16.shape[1]
    W1, W2 = weights(params, C)
    f = forward(lograd16, exposure, params)
    x, h = f["x16"], f["h"]
    y = y_saved.detach().cpu().double()
    dz = dy.detach().cpu().double() * y * (1 - y)               # (n,C)
    dh = dz[:, :, None] * W2[None, :, 0, :] * (h > 0)           # (n,C,64)
    tx = dh * W1[None, :, :, 0]
    out = {"dx": tx.sum(-1), "A_s": tx.abs().sum(-1)}
    k = torch.ones(x.shape[0], dtype=torch.bool) if keep is None else keep.cpu()
    dhk, dzk, xk, hk = dh[k], dz[k], x[k], h[k]
    g = torch.zeros(C, N_PARAMS, dtype=torch.float64)
    A = torch.zeros(C, N_PARAMS, dtype=torch.float64)
    for dst, terms in ((g, lambda t: t), (A, torch.abs)):
        w1 = dst[:, :1024].reshape(C, 64, 16)
        w1[:, :, 0] = terms(dhk * xk[:, :, None]).sum(0)
        w1[:, :, 1:] = terms(dhk).sum(0)[:, :, None]
        dst[:, 1024:1024 + 64] = terms(dzk[:, :, None] * hk).sum(0)
    out["g"], out["A"] = g.reshape(-1), A.reshape(-1)
    return out


def restatement(lograd, log_e, params, C):
    """The same network as differentiable fp64 torch on the padded row [x, 1, ..., 1] (two matmuls
    per channel); each rounding to half is applied to the value and passed straight through by the
    gradient.  lograd (n,C) fp64 (requires grad), log_e (n,1) fp64, params (C*2048) fp64 (requires
    grad, values already half-representable).  -> y (n,C)."""
    def rnd(t):
        return t + (t.detach().half().double() - t.detach())
    P = params.reshape(C, N_PARAMS)
    ys = []
    for c in range(C):
        W1, W2 = P[c, :1024].reshape(64, 16), P[c, 1024:].reshape(16, 64)
        s = lograd[:, c:c + 1] + log_e
        x = rnd(s + (s.detach().float().double() - s.detach()))  # the addition is fp32
        row = torch.cat([x, torch.ones(x.shape[0], 15, dtype=torch.float64)], 1)
        hid = rnd(torch.relu(row @ W1.t()))
        ys.append(torch.sigmoid(hid @ W2.t())[:, :1])
    return torch.cat(ys, 1)
