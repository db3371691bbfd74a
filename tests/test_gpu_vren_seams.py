"""The wave-per-ray compositing kernels, the loss kernels and the march's capacity clipping at their
seams, against the fp64 references of tests/composite_ref.py (csrc/vren_composite.hip, csrc/vren_march.hip).

The batch (composite_ref.seam_rays: 93 rays, 22 373 samples) has ray lengths around every multiple
of the 64-sample chunk, termination designed at lane 63, lane 0 of the next chunk, the last and the
last-but-one sample, permuted ray ids, shuffled segments with gaps between them, NaN in every input
gap and a sentinel in every output, so that a dropped carry between chunks, a row used for a ray id
or a store outside a ray's segment each fail a test.  The C ABI is called directly (mfnerf._lib.call):
the wrappers of mfnerf.vren zero-fill their outputs.

Tolerances.  E = max|x - ref64| / max|ref64| per output tensor over the batch.  A kernel's E must
stay within 8 x the E of the fp32 C oracle (oracle/vren_oracle.c) against the same fp64 reference
on the same inputs, computed by composite_ref.oracle_errors as tests/test_composite_ref_cpu.py does
(it also caps the oracle's E at 8e-6).  8 x covers __expf (hardware exp2, 1-2 ulp, where expf is
below 1), which the cancellation in 1 - exp(-x) at x = 2/1024 amplifies ~500 x, and tree-ordered
sums where the oracle's are sequential; a dropped carry or a wrong index is an O(1) error.  The
fused kernel's loss is one scalar, whose E is a single draw of rounding noise (the oracle chain's
came out at 1e-8 by luck), so its tolerance is 8 x E + 2^-18, the fp32 bound of the loss kernel
below.  mfnerf_nerf_loss has no C oracle; its bounds come from fp32 (half ulp 2^-24): each error
e = rgb + bg (1 - o) - gt carries 3 roundings of values below 2, |de| <= 6 * 2^-24 against
max|e| >= 0.5, plus 3 more for 2 e / 3n: gradients within 16 * 2^-24 = 2^-20 of their maximum; the
loss sums e^2 (relative error 2 de/e_rms plus <= 12 roundings of wave reduction and atomics):
within 64 * 2^-24 = 2^-18, plus 8 * 2^-24 of |loss_sum| for the accumulation onto a non-zero start.
total_samples, the march, fused against separate launches, sentinels and zeros are exact.

Measured (oracle E on the CPU -> tolerance 8 E; kernel E on an MI355X; every test prints them):
    output                   oracle E   tolerance  kernel E   kernel / oracle
    fw/opacity               1.637e-06  1.309e-05  2.962e-07  0.18
    fw/depth                 7.263e-07  5.811e-06  1.599e-06  2.20
    fw/rgb                   4.993e-07  3.994e-06  4.148e-07  0.83
    fw/ws                    2.895e-07  2.316e-06  6.992e-07  2.42
    bw/dL_dsigmas            1.236e-06  9.886e-06  1.089e-06  0.88
    bw/dL_drgbs              2.084e-07  1.667e-06  4.200e-07  2.02
    fused/dL_drgb            1.782e-06  1.426e-05  4.004e-07  0.22
    fused/dL_dopacity        1.704e-06  1.363e-05  2.408e-07  0.14
    fused/dL_dsigmas         8.598e-07  6.878e-06  6.527e-07  0.76
    fused/dL_drgbs           2.684e-07  2.147e-06  6.255e-07  2.33
    fused/loss               9.671e-09  3.892e-06  2.027e-08  (8 E + 2^-18)
    dist/loss                2.959e-06  2.367e-05  2.959e-06  1.00
    dist/ws_incl             6.002e-07  4.802e-06  6.002e-07  1.00
    dist/wts_incl            5.276e-07  4.221e-06  5.276e-07  1.00
    dist/dL_dws              5.473e-07  4.378e-06  5.473e-07  1.00
(fused: the same figures for n_mean = n_rays and 4 n_rays, the forward outputs as fw/; the distortion
kernels are the oracle's sequential loops and reproduce its figures digit for digit).  mfnerf_nerf_loss over its 10
cases: E(dL_drgb) <= 1.3e-7, E(dL_dopacity) <= 1.3e-7 against 9.5e-7; |loss - ref| <= 4.9e-8 against
>= 6.7e-7.  No kernel needed more than 2.5 of its 8 x.
"""
import functools

import pytest
import torch

import composite_ref as R
from mfnerf._lib import call, load, ptr, stream
from test_gpu_vren import aabb_hits, lego_inputs

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.9)
LAMBDA = 1e-3
SENT = -7.0
NAN = float("nan")
THR = R.T_THRESHOLD
EPS = 2.0 ** -24


def _check(name, got, want, tol):
    e = R.err(got.cpu(), want)
    print(f"kernel E {name:24s} {e:.3e}  (oracle {tol / 8:.3e}, tolerance {tol:.3e})")
    assert e <= tol, (name, e, tol)


@pytest.fixture(scope="module")
def seam(gpu, oracle):
    b = R.seam_rays(0)
    g = R.seam_grads(b)
    ra, in_ray = b["rays_a"], b["in_ray"]
    n_rays, n = ra.shape[0], in_ray.shape[0]
    s = dict(b=b, g=g, n_rays=n_rays, n=n, gap=~in_ray)
    s["E"] = R.oracle_errors(oracle, b, g, BG, LAMBDA, (n_rays, 4 * n_rays))
    s["ref"] = R.composite_fw64(b["sigmas"], b["rgbs"], b["deltas"], b["ts"], ra)
    s["after"] = R.after_termination(ra, s["ref"]["total"], n)
    s["dW"] = torch.where(in_ray, g["dW"], torch.tensor(NAN))  # gaps of this input hold NaN too
    s["dev"] = {k: b[k].to(gpu) for k in ("sigmas", "rgbs", "deltas", "ts", "rays_a")}
    return s


def _outs(s, gpu):
    """Every output prefilled: per-ray rows with NaN (each must be written), per-sample with SENT."""
    f32 = dict(dtype=torch.float32, device=gpu)
    n_rays, n = s["n_rays"], s["n"]
    return dict(total=torch.full((n_rays,), -7, dtype=torch.int64, device=gpu), op=torch.full((n_rays,), NAN, **f32),
                de=torch.full((n_rays,), NAN, **f32), rgb=torch.full((n_rays, 3), NAN, **f32),
                ws=torch.full((n,), SENT, **f32), g_rgb=torch.full((n_rays, 3), NAN, **f32),
                g_op=torch.full((n_rays,), NAN, **f32), dsig=torch.full((n,), SENT, **f32),
                drgb=torch.full((n, 3), SENT, **f32), loss=torch.full(((n_rays + 3) // 4,), NAN, **f32))


def _per_sample(s, x):
    """Checks the exact parts of a per-sample output (sentinel in the gaps, zeros after termination)
    and returns it on the CPU with the gaps zeroed, for the error measure."""
    x = x.cpu()
    assert (x[s["gap"]] == SENT).all(), "a gap sample was written"
    assert (x[s["after"]] == 0).all(), "non-zero after termination"
    assert s["after"].sum() > 5000
    x = x.clone()
    x[s["gap"]] = 0
    return x


def _fw(s, o):
    d = s["dev"]
    call("mfnerf_composite_train_fw", ptr(d["sigmas"]), ptr(d["rgbs"]), ptr(d["deltas"]), ptr(d["ts"]),
         ptr(d["rays_a"]), s["n_rays"], s["n"], THR, ptr(o["total"]), ptr(o["op"]), ptr(o["de"]), ptr(o["rgb"]),
         ptr(o["ws"]), stream())


def _bw(s, o, dO, dD, dC, dW):
    d = s["dev"]
    call("mfnerf_composite_train_bw", ptr(dO), ptr(dD), ptr(dC), ptr(dW), ptr(d["sigmas"]), ptr(d["rgbs"]),
         ptr(o["ws"]), ptr(d["deltas"]), ptr(d["ts"]), ptr(d["rays_a"]), ptr(o["op"]), ptr(o["de"]), ptr(o["rgb"]),
         s["n_rays"], s["n"], THR, ptr(o["dsig"]), ptr(o["drgb"]), stream())


def test_composite_fw_bw_on_seam_rays(gpu, seam):
    s, b, g, E = seam, seam["b"], seam["g"], seam["E"]
    o = _outs(s, gpu)
    _fw(s, o)
    torch.cuda.synchronize()
    ref = s["ref"]
    total = o["total"].cpu()
    assert torch.equal(total, ref["total"])  # every ray: none is ambiguous by construction
    N_by_ray = torch.zeros(s["n_rays"], dtype=torch.long)
    N_by_ray[b["rays_a"][:, 0]] = b["rays_a"][:, 2]
    assert torch.equal(total, torch.where(b["kill"] >= 0, b["kill"], N_by_ray))
    _check("fw/opacity", o["op"], ref["opacity"], 8 * E["fw/opacity"])
    _check("fw/depth", o["de"], ref["depth"], 8 * E["fw/depth"])
    _check("fw/rgb", o["rgb"], ref["rgb"], 8 * E["fw/rgb"])
    _check("fw/ws", _per_sample(s, o["ws"]), ref["ws"], 8 * E["fw/ws"])
    # backward: all four upstream gradients random and non-zero, read by ray id
    dO, dD, dC, dW = (t.to(gpu) for t in (g["dO"], g["dD"], g["dC"], s["dW"]))
    _bw(s, o, dO, dD, dC, dW)
    torch.cuda.synchronize()
    rs, rc = R.composite_bw64(g["dO"], g["dD"], g["dC"], g["dW"], b["sigmas"], b["rgbs"], b["deltas"], b["ts"],
                              b["rays_a"])
    _check("bw/dL_dsigmas", _per_sample(s, o["dsig"]), rs, 8 * E["bw/dL_dsigmas"])
    _check("bw/dL_drgbs", _per_sample(s, o["drgb"]), rc, 8 * E["bw/dL_drgbs"])


@pytest.mark.parametrize("mean_x", [1, 4])
def test_composite_fused_on_seam_rays(gpu, seam, mean_x):
    s, b, g, E = seam, seam["b"], seam["g"], seam["E"]
    d, n_rays, n = s["dev"], s["n_rays"], s["n"]
    n_mean = mean_x * n_rays
    target = g["target"].to(gpu)
    a = _outs(s, gpu)
    call("mfnerf_composite_train_fused", ptr(d["sigmas"]), ptr(d["rgbs"]), ptr(d["deltas"]), ptr(d["ts"]),
         ptr(d["rays_a"]), n_rays, n, THR, ptr(target), n_mean, LAMBDA, *BG, ptr(a["total"]), ptr(a["op"]),
         ptr(a["de"]), ptr(a["rgb"]), ptr(a["ws"]), ptr(a["g_rgb"]), ptr(a["g_op"]), ptr(a["dsig"]), ptr(a["drgb"]),
         ptr(a["loss"]), stream())
    # the three separate launches, bit for bit (dL_ddepth = dL_dws = 0)
    c = _outs(s, gpu)
    _fw(s, c)
    c["loss"] = torch.zeros(1, dtype=torch.float32, device=gpu)
    call("mfnerf_nerf_loss", ptr(c["rgb"]), ptr(c["op"]), ptr(target), n_rays, n_mean, LAMBDA, *BG, ptr(c["g_rgb"]),
         ptr(c["g_op"]), ptr(c["loss"]), stream())
    zr, zs = torch.zeros(n_rays, device=gpu), torch.zeros(n, device=gpu)
    _bw(s, c, c["g_op"], zr, c["g_rgb"], zs)
    torch.cuda.synchronize()
    for k in a:
        if k == "loss":
            la, lc = float(a[k].double().sum()), float(c[k])
            assert abs(la - lc) <= 1e-6 * abs(lc)
        else:
            assert torch.equal(a[k], c[k]), k
    # fp64: forward -> loss -> backward
    ref = s["ref"]
    l64, gc64, go64 = R.nerf_loss64(ref["rgb"], ref["opacity"], g["target"], n_mean, LAMBDA, BG)
    rs, rc = R.composite_bw64(go64, torch.zeros(n_rays), gc64, torch.zeros(n), b["sigmas"], b["rgbs"], b["deltas"],
                              b["ts"], b["rays_a"])
    p = f"fused{mean_x}/"
    assert torch.equal(a["total"].cpu(), ref["total"])
    _check(p + "opacity", a["op"], ref["opacity"], 8 * E["fw/opacity"])
    _check(p + "depth", a["de"], ref["depth"], 8 * E["fw/depth"])
    _check(p + "rgb", a["rgb"], ref["rgb"], 8 * E["fw/rgb"])
    _check(p + "ws", _per_sample(s, a["ws"]), ref["ws"], 8 * E["fw/ws"])
    _check(p + "dL_drgb", a["g_rgb"], gc64, 8 * E[p + "dL_drgb"])
    _check(p + "dL_dopacity", a["g_op"], go64, 8 * E[p + "dL_dopacity"])
    _check(p + "dL_dsigmas", _per_sample(s, a["dsig"]), rs, 8 * E[p + "dL_dsigmas"])
    _check(p + "dL_drgbs", _per_sample(s, a["drgb"]), rc, 8 * E[p + "dL_drgbs"])
    tol = 8 * E[p + "loss"] + 2.0 ** -18
    e = abs(float(a["loss"].double().sum()) - float(l64)) / abs(float(l64))
    print(f"kernel E {p + 'loss':24s} {e:.3e}  (oracle {E[p + 'loss']:.3e}, tolerance {tol:.3e})")
    assert e <= tol


@pytest.mark.parametrize("mean_x", [1, 4])
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 257])
def test_nerf_loss_against_fp64(gpu, n_rays, mean_x):
    g = torch.Generator().manual_seed(100 + n_rays)
    rgb, op = torch.rand(n_rays, 3, generator=g), torch.rand(n_rays, generator=g)
    gt = torch.rand(n_rays, 3, generator=g)
    op[-1] = 0.0            # opacity exactly 0 (o~ = 1e-10) ...
    if n_rays > 1:
        op[0] = 1.0         # ... and exactly 1 (ln o~ = 0 in fp32)
    n_mean, start, guard = mean_x * n_rays, 0.75, 64
    l64, c64, o64 = R.nerf_loss64(rgb, op, gt, n_mean, LAMBDA, BG)
    RGB, OP, GT = rgb.to(gpu), op.to(gpu), gt.to(gpu)
    outs = []
    for with_sum in (True, False):
        g_rgb = torch.full((n_rays + guard, 3), SENT, device=gpu)
        g_op = torch.full((n_rays + guard,), SENT, device=gpu)
        loss = torch.full((1,), start, device=gpu)  # accumulated into, not overwritten
        call("mfnerf_nerf_loss", ptr(RGB), ptr(OP), ptr(GT), n_rays, n_mean, LAMBDA, *BG, ptr(g_rgb), ptr(g_op),
             ptr(loss if with_sum else None), stream())
        torch.cuda.synchronize()
        assert (g_rgb[n_rays:] == SENT).all() and (g_op[n_rays:] == SENT).all()
        outs.append((g_rgb[:n_rays].cpu(), g_op[:n_rays].cpu(), float(loss)))
    (c, o, l), (c0, o0, l0) = outs
    assert l0 == start and torch.equal(c, c0) and torch.equal(o, o0)  # loss_sum = NULL: gradients only
    ec, eo = R.err(c, c64), R.err(o, o64)
    el, tol_l = abs(l - start - float(l64)), 64 * EPS * abs(float(l64)) + 8 * EPS * (start + abs(float(l64)))
    print(f"nerf_loss n={n_rays} n_mean={n_mean}: E dL_drgb {ec:.3e} dL_dopacity {eo:.3e} (tolerance {16 * EPS:.3e}); "
          f"|loss - ref| {el:.3e} (tolerance {tol_l:.3e})")
    assert ec <= 16 * EPS and eo <= 16 * EPS
    assert el <= tol_l


def test_distortion_loss_on_seam_rays(gpu, seam):
    s, b, g, E = seam, seam["b"], seam["g"], seam["E"]
    d, n_rays, n, gap = s["dev"], s["n_rays"], s["n"], s["gap"]
    ra = b["rays_a"]
    w32 = s["ref"]["ws"].float()
    ref = R.distortion64(w32, b["deltas"], b["ts"], ra, g["dloss"])
    W = torch.where(b["in_ray"], w32, torch.tensor(NAN)).to(gpu)
    loss = torch.full((n_rays,), NAN, device=gpu)
    wsi, wtsi, dws = (torch.full((n,), SENT, device=gpu) for _ in range(3))
    call("mfnerf_distortion_loss_fw", ptr(W), ptr(d["deltas"]), ptr(d["ts"]), ptr(d["rays_a"]), n_rays, n, ptr(loss),
         ptr(wsi), ptr(wtsi), stream())
    dl = g["dloss"].to(gpu)
    call("mfnerf_distortion_loss_bw", ptr(dl), ptr(wsi), ptr(wtsi), ptr(W), ptr(d["deltas"]), ptr(d["ts"]),
         ptr(d["rays_a"]), n_rays, n, ptr(dws), stream())
    torch.cuda.synchronize()
    loss, wsi, wtsi, dws = loss.cpu(), wsi.cpu(), wtsi.cpu(), dws.cpu()
    empty = ra[ra[:, 2] == 0, 0]
    assert empty.numel() == 1 and (loss[empty] == 0).all()
    # the scans are written for the rays' samples only; dL_dws is zero-filled by the call (mfnerf.h)
    assert (wsi[gap] == SENT).all() and (wtsi[gap] == SENT).all()
    assert (dws[gap] == 0).all()
    wsi[gap], wtsi[gap] = 0, 0
    _check("dist/loss", loss, ref["loss"], 8 * E["dist/loss"])
    _check("dist/ws_incl", wsi, ref["ws_incl"], 8 * E["dist/ws_incl"])
    _check("dist/wts_incl", wtsi, ref["wts_incl"], 8 * E["dist/wts_incl"])
    _check("dist/dL_dws", dws, ref["dL_dws"], 8 * E["dist/dL_dws"])


# ---------------------------------------------------------------- march: capacity clipping
MARCH = {"wave": dict(exp_step=0.0, scale=0.5, cascades=1, seed=13),          # march_wave + march_expand
         "thread": dict(exp_step=1 / 256, scale=1.0, cascades=2, seed=11)}    # march_count + march_write
N_MARCH, MAX_SAMPLES, GUARD = 300, 1024, 256  # 300 rays: beyond the scan's 256 threads, ragged last thread


@functools.lru_cache(maxsize=None)
def _march_case(path):
    from oracle import vren_oracle as oracle
    c = MARCH[path]
    o, d, bf, _ = lego_inputs(N_MARCH, seed=c["seed"], scale=c["scale"], cascades=c["cascades"])
    hits = aabb_hits(oracle, o, d, half=c["scale"])[:, 0].contiguous()
    noise = torch.rand(N_MARCH, generator=torch.Generator().manual_seed(3))
    ref = oracle.raymarching_train(o, d, hits, bf, c["cascades"], c["scale"], c["exp_step"], noise, 128, MAX_SAMPLES)
    return o, d, hits, bf, noise, ref


def _march(gpu, path, ins, hits_dev, hits_stride, capacity):
    """mfnerf_raymarching_train into sentinel-filled buffers of capacity + GUARD samples."""
    c = MARCH[path]
    o, d, bf, noise = ins
    f32 = dict(dtype=torch.float32, device=gpu)
    rays_a = torch.full((N_MARCH, 3), -7, dtype=torch.int64, device=gpu)
    xyzs, dirs = torch.full((capacity + GUARD, 3), SENT, **f32), torch.full((capacity + GUARD, 3), SENT, **f32)
    deltas, ts = torch.full((capacity + GUARD,), SENT, **f32), torch.full((capacity + GUARD,), SENT, **f32)
    counter = torch.full((2,), -7, dtype=torch.int32, device=gpu)
    ws = torch.empty(max(16, load().mfnerf_raymarching_train_workspace(N_MARCH, MAX_SAMPLES)), dtype=torch.uint8,
                     device=gpu)
    call("mfnerf_raymarching_train", ptr(o), ptr(d), ptr(hits_dev), hits_stride, ptr(bf), c["cascades"], c["scale"],
         c["exp_step"], ptr(noise), 128, MAX_SAMPLES, N_MARCH, capacity, ptr(rays_a), ptr(xyzs), ptr(dirs),
         ptr(deltas), ptr(ts), ptr(counter), ptr(ws), stream())
    torch.cuda.synchronize()
    return [t.cpu() for t in (rays_a, xyzs, dirs, deltas, ts, counter)]


@pytest.mark.parametrize("path", ["wave", "thread"])
def test_march_capacity_clipping(gpu, path):
    o, d, hits, bf, noise, ref = _march_case(path)
    ra_r, c_r = ref[0], ref[5]
    tot = int(c_r[0])
    start, count = ra_r[:, 1], ra_r[:, 2]
    assert tot == int(count.sum()) and tot > 1000
    mid = next(r for r in range(N_MARCH // 2, N_MARCH) if int(count[r]) >= 2)  # a middle ray to cut through
    assert 0 < int(start[mid]) < tot - int(count[mid]) and int(count[256:].sum()) > 0  # samples on both sides
    ins = [t.to(gpu) for t in (o, d, bf, noise)]
    H = hits.to(gpu)
    runs = {}
    for cap in (0, int(start[mid]), int(start[mid]) + 1, tot - 1, tot, tot + 1):
        ra, x, dd, de, t, cnt = runs[cap] = _march(gpu, path, ins, H, 2, cap)
        kept = min(tot, cap)
        assert cnt.tolist() == [kept, N_MARCH], cap
        assert torch.equal(ra[:, 0], torch.arange(N_MARCH))
        assert torch.equal(ra[:, 1], start.clamp(max=cap)), cap
        assert torch.equal(ra[:, 2], torch.minimum(count, cap - start).clamp(min=0)), cap
        for got, want in ((x, ref[1]), (dd, ref[2]), (de, ref[3]), (t, ref[4])):
            assert torch.equal(got[:kept], want[:kept]), cap         # the oracle's prefix, bit for bit
            assert (got[cap:] == SENT).all(), cap                    # nothing stored past the capacity
    # hits_t as row 0 of a (n, 3, 2) tensor: row stride 6
    wide = torch.full((N_MARCH, 3, 2), NAN)
    wide[:, 0] = hits
    out6 = _march(gpu, path, ins, wide.to(gpu), 6, tot + 1)
    for a, b in zip(out6, runs[tot + 1]):
        assert torch.equal(a, b)
