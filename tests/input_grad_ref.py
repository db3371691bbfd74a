"""fp64 references of the field's input gradients, shared by test_input_grad_cpu.py and
test_gpu_input_grad.py (test infrastructure, no test in here).

dL/dx of the grid encoding, term by term (include/mfnerf.h, mfnerf_grid_encode_bw_input):
    dL/dx_d = (1/x_range) sum_l scale_l sum_f dL_dout[l,f] sum_c sgn_d(c) prod_{e != d} wt_e(c) table[idx_c][f]
with pos = fmaf(scale_l, x01, 0.5) taken in fp32 exactly as the kernels do (level_geo), everything
after it in fp64, and the indices from oracle.field_oracle.grid_index.
"""
import math

import torch

from oracle import field_oracle as FO

B_HALF = math.exp(math.log(2048 * 0.5 / 16) / 15)  # per-level scale of the reference at scale = 0.5
KINDS = [("Hash", 1), ("MixedFeature", 2)]


def layouts(kind, n_tables, log2_T=14):
    """(oracle layout, library layout) of GridLayout(16, 2, log2_T, 16, b, kind, n_tables)."""
    from mfnerf.grid import GridLayout
    return (FO.GridLayout(16, 2, log2_T, 16, B_HALF, kind, n_tables),
            GridLayout(16, 2, log2_T, 16, B_HALF, kind, n_tables))


def random_table16(layout, seed=0):
    """An fp16 table with O(1) entries (so every level contributes): (n_params,) f16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(layout.n_params, generator=g).half()


def points(n, seed=0):
    """n points in [0,1]^3 (f32): uniform random, the first three rows replaced (n permitting) by the
    corners 0 and 1 and by (0.5, 0.25, 0.75)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g)
    special = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.25, 0.75]])
    k = min(n, 3)
    x[:k] = special[:k]
    return x


def normalise(x, x_min, x_range):
    """The kernels' x01 = (x - x_min) / x_range in fp32."""
    return (x.float() - torch.tensor(x_min, dtype=torch.float32)) / torch.tensor(x_range, dtype=torch.float32)


def _geo(layout, l, x01):
    """fp32 pos -> (g int64 (n,3), w fp64 (n,3)) of level l."""
    pos = (x01.double() * float(layout.scales[l]) + 0.5).float()  # one rounding: the fp32 fma
    g = torch.floor(pos)
    return g.to(torch.int64), (pos - g).double()


def dx_ref(x01, table16, dy, layout, x_range=1.0):
    """(ref, A), both (n,3) f64: the formula's sum and the sum of its terms' absolute values
    (L * 8 * F = 256 terms per component at L = 16, F = 2)."""
    n, F = x01.shape[0], layout.F
    tab = table16.double().view(-1, F)
    dy = dy.double().view(n, layout.L, F)
    ref = torch.zeros(n, 3, dtype=torch.float64)
    A = torch.zeros(n, 3, dtype=torch.float64)
    for l in range(layout.L):
        g, w = _geo(layout, l, x01)
        s = float(layout.scales[l]) / float(x_range)
        for c in range(8):
            bit = [(c >> d) & 1 for d in range(3)]
            idx = FO.grid_index(layout, l, g[:, 0] + bit[0], g[:, 1] + bit[1], g[:, 2] + bit[2]) + layout.offsets[l]
            v = tab[idx]  # (n, F)
            wt = [w[:, e] if bit[e] else 1 - w[:, e] for e in range(3)]
            for d in range(3):
                e0, e1 = [e for e in range(3) if e != d]
                coef = (1.0 if bit[d] else -1.0) * s * wt[e0] * wt[e1]
                for f in range(F):
                    term = coef * dy[:, l, f] * v[:, f]
                    ref[:, d] += term
                    A[:, d] += term.abs()
    return ref, A


def encode64(x01_64, table16, layout, x01_32):
    """A differentiable fp64 restatement of the encode at x01_64 (the cell g taken from the fp32
    pos of x01_32, as the kernels take it): (n, L*F) f64."""
    F = layout.F
    tab = table16.double().view(-1, F)
    outs = []
    for l in range(layout.L):
        g, _ = _geo(layout, l, x01_32)
        w = x01_64 * float(layout.scales[l]) + 0.5 - g.double()
        acc = torch.zeros(x01_64.shape[0], F, dtype=torch.float64)
        for c in range(8):
            bit = [(c >> d) & 1 for d in range(3)]
            idx = FO.grid_index(layout, l, g[:, 0] + bit[0], g[:, 1] + bit[1], g[:, 2] + bit[2]) + layout.offsets[l]
            wt = torch.ones(x01_64.shape[0], dtype=torch.float64)
            for e in range(3):
                wt = wt * (w[:, e] if bit[e] else 1 - w[:, e])
            acc = acc + wt[:, None] * tab[idx]
        outs.append(acc)
    return torch.cat(outs, 1)


def sh4_jacobian64(dn):
    """d SH4(dn) / d dn, (n,16,3) f64, by autograd of the oracle's SH on (dn + 1) / 2."""
    dn = dn.double().detach().requires_grad_(True)
    sh = FO.sh4((dn + 1) / 2)
    rows = [torch.autograd.grad(sh[:, k].sum(), dn, retain_graph=True)[0] for k in range(16)]
    return torch.stack(rows, 1)


def ddirs_from_dsh(dirs, dsh):
    """dL/dd (n,3) f64 from dL/dSH (n,16): J^T g in dn = d/|d|, then the normalisation's Jacobian."""
    d = dirs.double()
    nrm = d.norm(dim=1, keepdim=True)
    dn = d / nrm
    gdn = torch.einsum("nkd,nk->nd", sh4_jacobian64(dn), dsh.double())
    return (gdn - dn * (dn * gdn).sum(1, keepdim=True)) / nrm


def segmented_ref(dxyz, A, ts, ddirs, rays_a):
    """fp64 per-ray sums (dL_drays_o, dL_drays_d, bound terms (o, d)) of per-sample gradients."""
    R = rays_a.shape[0]
    o = torch.zeros(R, 3, dtype=torch.float64)
    d = torch.zeros(R, 3, dtype=torch.float64)
    Ao = torch.zeros(R, 3, dtype=torch.float64)
    Ad = torch.zeros(R, 3, dtype=torch.float64)
    t = ts.double()[:, None]
    for r in range(R):
        ray, s0, cnt = (int(v) for v in rays_a[r])
        sl = slice(s0, s0 + cnt)
        o[ray] = dxyz[sl].sum(0)
        d[ray] = (t[sl] * dxyz[sl] + ddirs[sl].double()).sum(0)
        Ao[ray] = A[sl].sum(0)
        Ad[ray] = (t[sl].abs() * A[sl] + ddirs[sl].double().abs()).sum(0)
    return o, d, Ao, Ad
