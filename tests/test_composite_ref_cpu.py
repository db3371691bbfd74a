"""The fp32 C oracle (oracle/vren_oracle.c) against the fp64 references of tests/composite_ref.py on
the designed seam batch.  It guards the reference itself (two independent computations, one with a
hand-derived backward, one with autograd, must agree to fp32 rounding) and measures the oracle's
own error E = max|x - ref64| / max|ref64| per output: 8 x E is the tolerance the GPU kernels are
held to in tests/test_gpu_vren_seams.py, whose docstring records the figures printed here."""
import ctypes

import pytest
import torch

import composite_ref as R

BG = (0.2, 0.5, 0.9)
LAMBDA = 1e-3
SENTINEL = -7.0

# Ceiling on the oracle's E.  Its longest sequential fp32 sum has 1024 terms: a random walk of
# sqrt(1024) * 2^-24 = 1.9e-6 relative, and 1 - exp(-x) at x = 2/1024 amplifies expf's half ulp by
# 1/x = 512 into 3e-5 of one weight, about 1/N of a ray's sums.  4x headroom over the random walk.
E_CEILING = 8e-6


@pytest.fixture(scope="module")
def batch():
    b = R.seam_rays(0)
    return b, R.seam_grads(b)


def test_seam_batch_is_the_designed_one(batch):
    b, _ = batch
    ra = b["rays_a"]
    n_rays, n = ra.shape[0], b["sigmas"].shape[0]
    assert n_rays == 93 and n == 22373 and int(b["in_ray"].sum()) == 22089
    assert sorted(ra[:, 0].tolist()) == list(range(n_rays)) and not torch.equal(ra[:, 0], torch.arange(n_rays))
    assert sorted(set(ra[:, 2].tolist())) == list(R.LENGTHS)
    # segments: disjoint, GAP samples apart, LEAD before the first, not in row order
    seg = sorted((s, N) for _, s, N in ra.tolist())
    assert seg[0][0] == R.LEAD and all(a[0] + a[1] + R.GAP == c[0] for a, c in zip(seg, seg[1:]))
    assert not torch.equal(torch.argsort(ra[:, 1]), torch.arange(n_rays))
    for k in ("sigmas", "deltas", "ts"):
        assert torch.isnan(b[k][~b["in_ray"]]).all() and torch.isfinite(b[k][b["in_ray"]]).all()
    # every seam of the issue is present: (N, kill) pairs
    pairs = {(N, int(b["kill"][ray])) for ray, _, N in ra.tolist()}
    for want in ((64, 63), (65, 64), (65, 63), (128, 127), (129, 128), (1, 0), (1, -1), (65, -1), (1024, 1023),
                 (1024, 1022), (193, 128), (0, -1)):
        assert want in pairs


def test_termination_is_unambiguous_and_where_designed(batch):
    b, _ = batch
    ra = b["rays_a"]
    ref = R.composite_fw64(b["sigmas"], b["rgbs"], b["deltas"], b["ts"], ra)
    for ray, s0, N in ra.tolist():
        k = int(b["kill"][ray])
        assert int(ref["total"][ray]) == (k if k >= 0 else N)
        if N:
            T = torch.cumprod(torch.exp(-(b["sigmas"][s0:s0 + N] * b["deltas"][s0:s0 + N]).double()), 0)
            live = T[:k] if k >= 0 else T
            assert live.numel() == 0 or float(live.min()) > 0.04           # 400 x the threshold
            assert k < 0 or float(T[k]) < 2.5e-9 * (float(T[k - 1]) if k else 1.0)


def test_autograd_backward_matches_finite_differences(batch):
    """The fp64 backward is what everything is measured against: check it against central
    differences of the fp64 forward on a short terminated ray."""
    b, g = batch
    ra = b["rays_a"]
    row = next(i for i, (ray, s0, N) in enumerate(ra.tolist()) if N == 65 and int(b["kill"][ray]) == 63)
    one = ra[row:row + 1]
    ray, s0, N = one[0].tolist()
    args = [b[k].double() for k in ("sigmas", "rgbs", "deltas", "ts")]
    dW = R.dense(g["dW"], b["in_ray"]).double()

    def scalar(sig):
        f = R.composite_fw64(sig, *args[1:], one)
        return float(g["dO"][ray] * f["opacity"][ray] + g["dD"][ray] * f["depth"][ray]
                     + (g["dC"][ray].double() * f["rgb"][ray]).sum() + (dW[s0:s0 + N] * f["ws"][s0:s0 + N]).sum())
    ds, _ = R.composite_bw64(g["dO"], g["dD"], g["dC"], dW, *args, one)
    for k in (0, 31, 62, 63, 64):
        h = 1e-6 * float(args[0][s0 + k])
        p, m = args[0].clone(), args[0].clone()
        p[s0 + k] += h
        m[s0 + k] -= h
        fd = (scalar(p) - scalar(m)) / (2 * h)
        assert abs(fd - float(ds[s0 + k])) <= 1e-6 * float(ds[s0:s0 + N].abs().max()), k
    assert float(ds[s0 + 64]) == 0.0  # past the termination


def test_oracle_against_fp64_on_seam_rays(batch, oracle):
    b, g = batch
    E = R.oracle_errors(oracle, b, g, BG, LAMBDA, (93, 4 * 93))   # asserts total_samples inside
    for k, v in E.items():
        print(f"oracle E {k:24s} {v:.3e}")
    for k, v in E.items():
        assert v <= E_CEILING, (k, v)


def test_oracle_leaves_gaps_and_zeros_after_termination(batch, oracle):
    """The C functions called on sentinel-filled per-sample outputs: segment samples are written
    (exact zeros after termination come from the zero-fill the reference relies on, so here they
    keep the sentinel too), gap samples are never touched."""
    b, g = batch
    ra, gap = b["rays_a"], ~b["in_ray"]
    n_rays, n = ra.shape[0], b["sigmas"].shape[0]
    ins = [R.dense(b[k], b["in_ray"]) for k in ("sigmas", "rgbs", "deltas", "ts")]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tot, op, de = torch.zeros(n_rays, dtype=torch.long), torch.zeros(n_rays), torch.zeros(n_rays)
    rgb, ws = torch.zeros(n_rays, 3), torch.full((n,), SENTINEL)
    oracle.lib().orc_composite_train_fw(n_rays, *[p(t) for t in ins], p(ra), R.T_THRESHOLD, p(tot), p(op), p(de),
                                        p(rgb), p(ws))
    ref = R.composite_fw64(*ins, ra)
    after = R.after_termination(ra, ref["total"], n)
    assert after.sum() > 5000
    assert (ws[gap | after] == SENTINEL).all() and (ws[~(gap | after)] != SENTINEL).all()
    dW = R.dense(g["dW"], b["in_ray"])
    ws0 = torch.where(ws == SENTINEL, torch.zeros(()), ws)
    ds, dc, scratch = torch.full((n,), SENTINEL), torch.full((n, 3), SENTINEL), torch.zeros(n)
    oracle.lib().orc_composite_train_bw(n_rays, p(g["dO"]), p(g["dD"]), p(g["dC"]), p(dW), p(ins[0]), p(ins[1]),
                                        p(ws0), p(ins[2]), p(ins[3]), p(ra), p(op), p(de), p(rgb), R.T_THRESHOLD,
                                        p(scratch), p(ds), p(dc))
    assert (ds[gap | after] == SENTINEL).all() and (dc[gap | after] == SENTINEL).all()
    assert (ds[~(gap | after)] != SENTINEL).all()


@pytest.mark.parametrize("n_rays", [1, 65, 257])
def test_nerf_loss_fp32_restatement_against_fp64(n_rays):
    """nerf_loss32 (the oracle chain's middle stage) within the fp32 bounds the GPU kernel is held to."""
    g = torch.Generator().manual_seed(n_rays)
    rgb, op = torch.rand(n_rays, 3, generator=g), torch.rand(n_rays, generator=g)
    gt = torch.rand(n_rays, 3, generator=g)
    op[0] = 1.0
    op[-1] = 0.0
    for nm in (n_rays, 4 * n_rays):
        l64, c64, o64 = R.nerf_loss64(rgb, op, gt, nm, LAMBDA, BG)
        l32, c32, o32 = R.nerf_loss32(rgb, op, gt, nm, LAMBDA, BG)
        assert abs(float(l32) - float(l64)) <= 2.0 ** -18 * abs(float(l64))
        assert R.err(c32, c64) <= 2.0 ** -20 and R.err(o32, o64) <= 2.0 ** -20
