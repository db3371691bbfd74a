"""Camera-pose refinement, the reference's --optimize_ext (train.py:91-94, 122-139, opt.py:47).

Every training image gets a rotation offset dR (axis-angle) and a translation offset dT, both zero
at the start, applied to its camera-to-world pose before the rays are formed; they train beside the
field from the loss gradient with respect to the rays, which the field's input gradients provide
(mfnerf.field: mfnerf_field_bw_inputs, mfnerf_grid_encode_bw_input, summed per ray by
RayMarcher.backward).

    refiner = PoseRefiner(len(poses)).to(device)
    rays_o, rays_d = data.get_rays(directions, refiner(poses[img_idxs], img_idxs))
    loss(render(model, rays_o, rays_d)).backward()      # refiner.dR.grad, refiner.dT.grad

The fused step trains the same offsets inside its graphs (engine.StepConfig(refine_poses=True),
trainer.HParams(optimize_ext=True); csrc/pose.hip); fused_offsets() / fused_refined_poses() read them.
"""
import torch
from torch import nn

POSE_LR = 1e-6  # train.py:139 hard-codes it


def axisangle_to_R(v):
    """Rodrigues' formula (ray_utils.py:74-100): axis-angle v (3) or (B,3) -> R (3,3) or (B,3,3),
    R = I + sin(t)/t K + (1 - cos(t))/t^2 K^2 with K the skew matrix of v and t = |v| + 1e-7 (the
    reference's guard at v = 0).  fp32 whatever autocast says, as the reference decorates it."""
    with torch.autocast(v.device.type, enabled=False):
        single = v.ndim == 1
        w = v.float().reshape(-1, 3)
        wx, wy, wz = w.unbind(-1)
        o = torch.zeros_like(wx)
        K = torch.stack([o, -wz, wy, wz, o, -wx, -wy, wx, o], -1).reshape(-1, 3, 3)
        t = (w.norm(dim=1) + 1e-7)[:, None, None]
        R = torch.eye(3, device=v.device) + (torch.sin(t) / t) * K + ((1 - torch.cos(t)) / (t * t)) * (K @ K)
        return R[0] if single else R


class PoseRefiner(nn.Module):
    """dR, dT (n_images, 3), zero-initialised parameters (train.py:122-128)."""

    def __init__(self, n_images):
        super().__init__()
        self.dR = nn.Parameter(torch.zeros(n_images, 3))
        self.dT = nn.Parameter(torch.zeros(n_images, 3))

    def forward(self, poses, img_idxs):
        """train.py:91-94 on poses (B,3,4) of the images img_idxs (B): the rotation offset is applied
        on the left of the whole 3x3 block, the translation offset added.  The input is not modified."""
        dR = axisangle_to_R(self.dR[img_idxs])
        rot = dR @ poses[..., :3].to(dR.dtype)
        trans = poses[..., 3].to(dR.dtype) + self.dT[img_idxs]
        return torch.cat([rot, trans[..., None]], -1)

    def refined_poses(self, poses):
        """Every image's refined pose (n_images,3,4), detached: what a checkpoint saves beside dR and
        dT (train.py:295, save_poses)."""
        with torch.no_grad():
            return self(poses, torch.arange(self.dR.shape[0], device=self.dR.device))

    def optimizer(self, lr=POSE_LR):
        """The reference's second optimizer (train.py:139): Adam over [dR, dT] at a fixed 1e-6."""
        return torch.optim.Adam([self.dR, self.dT], lr)


# ---------------------------------------------------------------------------- the fused step's poses
def fused_offsets(step):
    """(dR, dT), each (n_images, 3): the offsets an engine.TrainStep(StepConfig(refine_poses=True))
    trains, the device tensors themselves (read them after a synchronisation; the step's kernels
    update them in place)."""
    if not step.cfg.refine_poses or getattr(step, "dR", None) is None:
        raise ValueError("the step does not refine poses (StepConfig.refine_poses with an attached dataset)")
    return step.dR, step.dT


def fused_refined_poses(step):
    """[R(dR) @ R0 | t0 + dT] of every image (n_images,3,4) from the step's current offsets: forward()
    of a PoseRefiner holding them."""
    dR, dT = fused_offsets(step)
    ref = PoseRefiner(dR.shape[0]).to(dR.device)
    with torch.no_grad():
        ref.dR.copy_(dR)
        ref.dT.copy_(dT)
    return ref.refined_poses(step.dataset.poses)
