"""fp64 references of the pose-refinement kernels (mfnerf_pose_grad, mfnerf_pose_step): the
reference's axisangle_to_R (datasets/ray_utils.py; R(w) = I + sin(t)/t K + (1 - cos t)/t^2 K^2,
t = |w| + 1e-7), the analytic transposed Jacobian of w -> R(w) u, the per-image reduction of the ray
gradients and torch Adam, all in torch float64 on the CPU.  Inputs are the fp32 values the kernels
read, widened."""
import torch

GUARD = 1e-7


def skew(w):
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(*w.shape[:-1], 3, 3)


def rotation(w):
    """R(w) (...,3,3) fp64, differentiable (the formula itself: what autograd differentiates)."""
    w = w.double()
    K = skew(w)
    t = (w.norm(dim=-1) + GUARD)[..., None, None]
    eye = torch.eye(3, dtype=torch.float64)
    return eye + (torch.sin(t) / t) * K + ((1 - torch.cos(t)) / (t * t)) * (K @ K)


def rotate(w, u):
    """R(w) u for w (...,3), u (...,3)."""
    return (rotation(w) @ u.double()[..., None])[..., 0]


def compose(poses, dR, dT):
    """[R(dR[i]) @ R0[i] | t0[i] + dT[i]] (n,3,4) fp64."""
    p = poses.double()
    return torch.cat([rotation(dR) @ p[..., :3], (p[..., 3] + dT.double())[..., None]], -1)


def jt_g(w, u, g):
    """J(w, u)^T g (...,3) fp64, J the Jacobian of w -> R(w) u, written out:
        a (u x g) + b ((w x u) x g + u x (g x w)) + (w/|w|) (a' g.(w x u) + b' g.(w x (w x u)))
    with a = sin t / t, b = (1 - cos t)/t^2, a' = (t cos t - sin t)/t^2, b' = (t sin t - 2(1 - cos t))/t^3
    and d|w|/dw = 0 at w = 0.  fp64 holds the closed forms of a', b' down to t = 1e-7 only to ~1e-2
    relative (b': a difference of 1e-14 terms that leaves 1e-29), so under t = 1e-2 they are their
    series (next terms < 1e-18 relative); both enter scaled by |w| <= t, |w|^2."""
    w, u, g = w.double(), u.double(), g.double()
    n = w.norm(dim=-1, keepdim=True)
    t = n + GUARD
    unit = torch.where(n > 0, w / n.clamp_min(1e-300), torch.zeros_like(w))
    a = torch.sin(t) / t
    b = 2 * torch.sin(t / 2) ** 2 / (t * t)
    da_c = (t * torch.cos(t) - torch.sin(t)) / (t * t)
    db_c = (t * torch.sin(t) - 4 * torch.sin(t / 2) ** 2) / t ** 3
    t2 = t * t
    da_s = t * (-1 / 3 + t2 * (1 / 30 - t2 * (1 / 840 - t2 / 45360)))
    db_s = t * (-1 / 12 + t2 * (1 / 180 - t2 * (1 / 6720 - t2 / 403200)))
    small = t < 1e-2
    da, db = torch.where(small, da_s, da_c), torch.where(small, db_s, db_c)
    cr = torch.linalg.cross
    c = cr(w, u)
    radial = da * (g * c).sum(-1, keepdim=True) + db * (g * cr(w, c)).sum(-1, keepdim=True)
    return a * cr(u, g) + b * (cr(c, g) + cr(u, cr(g, w))) + unit * radial


def base_dirs(poses, directions, img_idx, pix_idx):
    """u_r = R0[img_r] @ directions[pix_r] (n_rays,3) fp64."""
    R0 = poses.double()[img_idx.long(), :, :3]
    return (R0 @ directions.double()[pix_idx.long()][..., None])[..., 0]


def pose_grad(g_o, g_d, img_idx, pix_idx, poses, directions, dR):
    """(grad_dR, grad_dT, A_dR, A_dT), each (n_img,3) fp64 except the bounds' sums A (n_img):
    A_dR[i] = sum_r |u_r| |g_d_r| and A_dT[i] = sum_r |g_o_r| over the rays of image i."""
    n_img = poses.shape[0]
    idx = img_idx.long()
    u = base_dirs(poses, directions, img_idx, pix_idx)
    j = jt_g(dR.double()[idx], u, g_d)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    gR = z(n_img, 3).index_add_(0, idx, j)
    gT = z(n_img, 3).index_add_(0, idx, g_o.double())
    A_R = z(n_img).index_add_(0, idx, u.norm(dim=1) * g_d.double().norm(dim=1))
    A_T = z(n_img).index_add_(0, idx, g_o.double().norm(dim=1))
    return gR, gT, A_R, A_T


class Adam64:
    """torch.optim.Adam's update (betas, eps, lr given as the fp32 values the C ABI carries, widened)
    in fp64 over one tensor; keeps sum |update| for the parameter bound and m over |g| for m's."""

    def __init__(self, p, lr, b1=0.9, b2=0.999, eps=1e-8):
        f = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
        self.lr, self.b1, self.b2, self.eps = f(lr), f(b1), f(b2), f(eps)
        self.p = p.double().clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.m_abs = torch.zeros_like(self.p)
        self.moved = torch.zeros_like(self.p)
        self.t = 0

    def step(self, g):
        g = g.double()
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.m_abs = self.b1 * self.m_abs + (1 - self.b1) * g.abs()
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        upd = self.lr * (self.m / bc1) / ((self.v / bc2).sqrt() + self.eps)
        self.p = self.p - upd
        self.moved += upd.abs()
        return self.p
