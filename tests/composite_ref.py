"""fp64 references of the `vren` compositing, distortion-loss and NeRF-loss kernels, and the designed
batch that puts every seam of the wave-per-ray kernels (64-sample chunks, carries between chunks,
termination at a chunk edge) under test.  CPU, torch only.

The forward is volumerendering.cu:6-45 in torch float64; every backward here is torch autograd of
the fp64 forward (the termination mask held constant), NOT a restatement of the hand-derived
formulas the kernels and oracle/vren_oracle.c share.  Inputs are the fp32 values the kernels read,
widened.  Per-ray outputs are indexed by ray id (rays_a[:, 0]), as the kernels index them."""
import torch

T_THRESHOLD = 1e-4
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1024)
GAP, LEAD = 3, 5  # samples between segments / before the first one


def _kills(N):
    """Termination samples tried for a ray of N samples: None (runs to its end), then each seam."""
    ks = sorted({k for k in (0, 1, 62, 63, 64, 65, 127, 128, N - 2, N - 1) if 0 <= k < N})
    return [None] + ks


def seam_rays(seed=0):
    """The designed batch -> dict(rays_a, sigmas, rgbs, deltas, ts, kill, in_ray).

    One ray per (length, termination sample).  delta ~ U(0.001, 0.005); an ordinary sample has
    sigma*delta = u * 2/N, u ~ U(0.5, 1.5), so T stays above exp(-3) > 0.04 over a whole ray; the
    kill sample has sigma*delta = 20, after which T <= 2.1e-9: termination is never within a factor
    400 of T_THRESHOLD, so total_samples is unambiguous for every ray.  rays_a[:, 0] is a random
    permutation of the ray ids; the segments lie in shuffled order, LEAD samples before the first
    and GAP samples after each.  Gap samples of every input hold NaN (no kernel may read them).
    kill[ray id] = the sample at which that ray terminates, -1 for none; in_ray marks segment samples."""
    g = torch.Generator().manual_seed(seed)
    spec = [(N, k) for N in LENGTHS for k in _kills(N)]
    n_rays = len(spec)
    ids = torch.randperm(n_rays, generator=g)       # row -> ray id
    order = torch.randperm(n_rays, generator=g)     # storage order of the rows' segments
    start = torch.zeros(n_rays, dtype=torch.long)
    pos = LEAD
    for row in order.tolist():
        start[row] = pos
        pos += spec[row][0] + GAP
    n = pos
    nan = float("nan")
    sigmas, deltas, ts = torch.full((n,), nan), torch.full((n,), nan), torch.full((n,), nan)
    rgbs = torch.full((n, 3), nan)
    in_ray = torch.zeros(n, dtype=torch.bool)
    kill = torch.full((n_rays,), -1, dtype=torch.long)
    for row, (N, k) in enumerate(spec):
        s0 = int(start[row])
        kill[ids[row]] = -1 if k is None else k
        if N == 0:
            continue
        d = torch.rand(N, generator=g) * 0.004 + 0.001
        sd = (torch.rand(N, generator=g) + 0.5) * (2.0 / N)
        if k is not None:
            sd[k] = 20.0
        deltas[s0:s0 + N] = d
        sigmas[s0:s0 + N] = sd / d
        ts[s0:s0 + N] = 0.3 + torch.cumsum(d, 0) - 0.5 * d
        rgbs[s0:s0 + N] = torch.rand(N, 3, generator=g)
        in_ray[s0:s0 + N] = True
    rays_a = torch.stack([ids, start, torch.tensor([N for N, _ in spec])], 1).contiguous()
    return dict(rays_a=rays_a, sigmas=sigmas, rgbs=rgbs, deltas=deltas, ts=ts, kill=kill, in_ray=in_ray)


def after_termination(rays_a, total_samples, n_samples):
    """Mask of the segment samples past their ray's last accumulated one (index > total_samples)."""
    m = torch.zeros(n_samples, dtype=torch.bool)
    for ray, s0, N in rays_a.tolist():
        m[s0 + int(total_samples[ray]) + 1:s0 + N] = True
    return m


def _ray64(sig, rgb, dl, t, thr):
    """One ray in fp64 -> (total_samples, L = samples accumulated, w[:L], O, D, C); differentiable."""
    N = sig.shape[0]
    a = 1 - torch.exp(-sig * dl)
    T_after = torch.cumprod(1 - a, 0)
    hit = (T_after.detach() <= thr).nonzero()
    total = int(hit[0]) if hit.numel() else N
    L = min(total + 1, N)  # the terminating sample is accumulated too
    T_before = torch.cat([T_after.new_ones(1), T_after[:L - 1]])
    w = a[:L] * T_before
    return total, L, w, w.sum(), (w * t[:L]).sum(), (w[:, None] * rgb[:L]).sum(0)


def composite_test64(sigmas, rgbs, deltas, ts, n_eff, thr=T_THRESHOLD):
    """Test-time compositing (volumerendering.cu:206-249 from opacity 0) in fp64 on the row-per-ray
    layout of raymarching_test: sigmas, deltas, ts (n, S), rgbs (n, S, 3), n_eff (n) samples per row.
    A sample is accumulated, then the ray stops when T <= thr (the terminating sample counts).
    -> (opacity (n), depth (n), rgb (n, 3) fp64, count (n) int64 = samples accumulated)."""
    S = sigmas.shape[1]
    n_eff = n_eff.long()
    if S == 0:
        z = torch.zeros(sigmas.shape[0], dtype=torch.float64)
        return z, z.clone(), torch.zeros(sigmas.shape[0], 3, dtype=torch.float64), n_eff.clone()
    live = torch.arange(S)[None] < n_eff[:, None]
    a = torch.where(live, 1 - torch.exp(-sigmas.double() * deltas.double()), torch.zeros((), dtype=torch.float64))
    T_after = torch.cumprod(1 - a, 1)
    stop = live & (T_after <= thr)
    first = torch.where(stop.any(1), stop.int().argmax(1), torch.full_like(n_eff, S))
    count = torch.minimum(first + 1, n_eff)
    T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], 1)
    w = torch.where(torch.arange(S)[None] < count[:, None], a * T_before, torch.zeros((), dtype=torch.float64))
    return w.sum(1), (w * ts.double()).sum(1), (w[:, :, None] * rgbs.double()).sum(1), count


def composite_fw64(sigmas, rgbs, deltas, ts, rays_a, thr=T_THRESHOLD):
    """-> dict(total int64, opacity, depth, rgb fp64 by ray id, ws fp64 per sample: 0 after
    termination and in the gaps)."""
    n_rays, n = max(rays_a.shape[0], int(rays_a[:, 0].max()) + 1), sigmas.shape[0]  # (a subset of the rows works too)
    S, C, Dl, Tt = sigmas.double(), rgbs.double(), deltas.double(), ts.double()
    out = dict(total=torch.zeros(n_rays, dtype=torch.long), opacity=torch.zeros(n_rays, dtype=torch.float64),
               depth=torch.zeros(n_rays, dtype=torch.float64), rgb=torch.zeros(n_rays, 3, dtype=torch.float64),
               ws=torch.zeros(n, dtype=torch.float64))
    for ray, s0, N in rays_a.tolist():
        if N == 0:
            continue
        sl = slice(s0, s0 + N)
        total, L, w, O, D, col = _ray64(S[sl], C[sl], Dl[sl], Tt[sl], thr)
        out["total"][ray], out["opacity"][ray], out["depth"][ray], out["rgb"][ray] = total, O, D, col
        out["ws"][s0:s0 + L] = w
    return out


def composite_bw64(dL_dopacity, dL_ddepth, dL_drgb, dL_dws, sigmas, rgbs, deltas, ts, rays_a, thr=T_THRESHOLD):
    """Autograd of L = sum dL_dopacity*O + dL_ddepth*D + dL_drgb.C + dL_dws.w through the fp64
    forward -> (dL_dsigmas (n), dL_drgbs (n,3)) fp64, zero after termination and in the gaps."""
    n = sigmas.shape[0]
    gO, gD, gC, gW = dL_dopacity.double(), dL_ddepth.double(), dL_drgb.double(), dL_dws.double()
    Dl, Tt = deltas.double(), ts.double()
    dsig, drgb = torch.zeros(n, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64)
    for ray, s0, N in rays_a.tolist():
        if N == 0:
            continue
        sl = slice(s0, s0 + N)
        sig = sigmas[sl].double().clone().requires_grad_(True)
        col = rgbs[sl].double().clone().requires_grad_(True)
        _, L, w, O, D, C = _ray64(sig, col, Dl[sl], Tt[sl], thr)
        loss = gO[ray] * O + gD[ray] * D + (gC[ray] * C).sum() + (gW[s0:s0 + L] * w).sum()
        dsig[sl], drgb[sl] = torch.autograd.grad(loss, (sig, col))
    return dsig, drgb


def distortion64(ws, deltas, ts, rays_a, dL_dloss=None):
    """Distortion loss from its O(N^2) definition, sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 d_i
    (tests/test_cpu.py::test_distortion_loss_definition), per ray in fp64 -> dict(loss by ray id,
    ws_incl, wts_incl per sample, and, given dL_dloss (by ray id), dL_dws by autograd)."""
    n_rays, n = rays_a.shape[0], ws.shape[0]
    out = dict(loss=torch.zeros(n_rays, dtype=torch.float64), ws_incl=torch.zeros(n, dtype=torch.float64),
               wts_incl=torch.zeros(n, dtype=torch.float64), dL_dws=torch.zeros(n, dtype=torch.float64))
    for ray, s0, N in rays_a.tolist():
        if N == 0:
            continue
        sl = slice(s0, s0 + N)
        w = ws[sl].double().clone().requires_grad_(True)
        t, d = ts[sl].double(), deltas[sl].double()
        loss = (w[:, None] * w[None] * (t[:, None] - t[None]).abs()).sum() + (w * w * d).sum() / 3
        out["loss"][ray] = loss.detach()
        out["ws_incl"][sl] = torch.cumsum(w.detach(), 0)
        out["wts_incl"][sl] = torch.cumsum(w.detach() * t, 0)
        if dL_dloss is not None:
            out["dL_dws"][sl], = torch.autograd.grad(dL_dloss[ray].double() * loss, w)
    return out


def nerf_loss64(rgb, opacity, target, n_mean, lambda_o, bg):
    """pred = rgb + bg*(1-o); loss = sum (pred-gt)^2 / (3 n_mean) + lambda * sum(-o~ ln o~) / n_mean,
    o~ = o + 1e-10 (losses.py:47-60 with train.py's background blend), fp64; bg a 3-vector.
    -> (loss, dL_drgb (n,3), dL_dopacity (n)) with the gradients by autograd."""
    c = rgb.double().clone().requires_grad_(True)  # (a copy: the caller's tensor stays a plain one)
    o = opacity.double().clone().requires_grad_(True)
    pred = c + torch.as_tensor(bg, dtype=torch.float64)[None] * (1 - o[:, None])
    ot = o + 1e-10
    loss = ((pred - target.double()) ** 2).sum() / (3 * n_mean) + lambda_o * (-ot * torch.log(ot)).sum() / n_mean
    g_c, g_o = torch.autograd.grad(loss, (c, o))
    return loss.detach(), g_c, g_o


def nerf_loss32(rgb, opacity, target, n_mean, lambda_o, bg):
    """The same loss and its hand-written gradient evaluated in plain fp32: the middle stage of the
    all-fp32 oracle chain (C oracle forward -> this -> C oracle backward) whose distance from the fp64
    chain sets the tolerance of the fused kernel."""
    f = torch.float32
    b = torch.tensor(bg, dtype=f)[None]
    inv3n, invn = torch.tensor(1.0, dtype=f) / (3.0 * n_mean), torch.tensor(1.0, dtype=f) / n_mean
    e = rgb + b * (1 - opacity[:, None]) - target
    g_c = 2 * e * inv3n
    o = opacity + 1e-10
    loss = (e * e * inv3n).sum() + (lambda_o * (-o * torch.log(o)) * invn).sum()
    g_o = -(b * g_c).sum(1) + lambda_o * (-(torch.log(o) + 1)) * invn
    return loss, g_c, g_o


def err(x, ref):
    """E = max|x - ref64| / max|ref64| over the whole tensor (per batch, not per ray)."""
    ref = ref.double()
    return float((x.double() - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------- the oracle's own error
def seam_grads(b, seed=1):
    """Random non-zero upstream gradients for the seam batch (per ray by ray id, dL_dws per sample)."""
    g = torch.Generator().manual_seed(seed)
    n_rays, n = b["rays_a"].shape[0], b["sigmas"].shape[0]
    return dict(dO=torch.randn(n_rays, generator=g), dD=torch.randn(n_rays, generator=g),
                dC=torch.randn(n_rays, 3, generator=g), dW=torch.randn(n, generator=g),
                target=torch.rand(n_rays, 3, generator=g), dloss=torch.randn(n_rays, generator=g))


def dense(t, in_ray):
    """A copy of a per-sample tensor with its gap samples (NaN in the designed batch) set to 0."""
    t = t.clone()
    t[~in_ray] = 0
    return t


def oracle_errors(oracle, b, g, bg, lambda_o, n_means):
    """E of the fp32 C oracle (oracle/vren_oracle.c) against the fp64 references on batch b with the
    upstream gradients g -> {name: E}.  Keys: fw/<out>, bw/<out>, fused<n_mean>/<out>, dist/<out>.
    8x these figures are the GPU kernels' tolerances (tests/test_gpu_vren_seams.py)."""
    ra, thr = b["rays_a"], T_THRESHOLD
    ins = [dense(b[k], b["in_ray"]) for k in ("sigmas", "rgbs", "deltas", "ts")]
    E = {}
    ref = composite_fw64(*ins, ra, thr)
    tot, op, de, rgb, ws = oracle.composite_train_fw(*ins, ra, thr)
    assert torch.equal(tot, ref["total"])
    for k, v in (("opacity", op), ("depth", de), ("rgb", rgb), ("ws", ws)):
        E["fw/" + k] = err(v, ref[k])
    # backward with every upstream gradient live; the forward values it reads are the oracle's own
    dW = dense(g["dW"], b["in_ray"])
    rs, rc = composite_bw64(g["dO"], g["dD"], g["dC"], dW, *ins, ra, thr)
    ds, dc = oracle.composite_train_bw(g["dO"], g["dD"], g["dC"], dW, ins[0], ins[1], ws, ins[2], ins[3], ra, op, de,
                                       rgb, thr)
    E["bw/dL_dsigmas"], E["bw/dL_drgbs"] = err(ds, rs), err(dc, rc)
    # the fused chain: forward -> NeRF loss -> backward with dL_ddepth = dL_dws = 0
    n_rays, n = ra.shape[0], ins[0].shape[0]
    for nm in n_means:
        l64, gc64, go64 = nerf_loss64(ref["rgb"], ref["opacity"], g["target"], nm, lambda_o, bg)
        rs, rc = composite_bw64(go64, torch.zeros(n_rays), gc64, torch.zeros(n), *ins, ra, thr)
        l32, gc32, go32 = nerf_loss32(rgb, op, g["target"], nm, lambda_o, bg)
        ds, dc = oracle.composite_train_bw(go32, torch.zeros(n_rays), gc32, torch.zeros(n), ins[0], ins[1], ws, ins[2],
                                           ins[3], ra, op, de, rgb, thr)
        p = f"fused{nm // n_rays}/"
        E[p + "loss"] = abs(float(l32) - float(l64)) / abs(float(l64))
        E[p + "dL_drgb"], E[p + "dL_dopacity"] = err(gc32, gc64), err(go32, go64)
        E[p + "dL_dsigmas"], E[p + "dL_drgbs"] = err(ds, rs), err(dc, rc)
    # distortion loss on the fp64 forward's weights rounded to fp32
    w32 = ref["ws"].float()
    r = distortion64(w32, ins[2], ins[3], ra, g["dloss"])
    loss, wsi, wtsi = oracle.distortion_loss_fw(w32, ins[2], ins[3], ra)
    dws = oracle.distortion_loss_bw(g["dloss"], wsi, wtsi, w32, ins[2], ins[3], ra)
    for k, v in (("loss", loss), ("ws_incl", wsi), ("wts_incl", wtsi), ("dL_dws", dws)):
        E["dist/" + k] = err(v, r[k])
    return E
