"""The fused MI355X training step: one NeRF training iteration of the reference's hot path
(train.py:164-190 -> rendering.py:121-163 -> losses.py:47-60 -> backward -> FusedAdam) as a
fixed set of gfx950 kernels with every intermediate resident in HBM and the sample counts kept on
the device (no host synchronisation, so a step is capturable in HIP graphs).

Parts.  The batch's rays are split into `n_parts` equal, independent ray ranges ("parts"): each
part is marched into its own sample buffers (own device counter, own rays_a) and runs its own
encode -> field -> composite -> loss -> backward chain; the loss of every part is normalised by the
FULL batch size (mfnerf_nerf_loss n_mean), so the parts' gradients add up to exactly the
full batch's.  Parts exist so that the chain of part p+1 (MFMA/VALU work) runs on another stream
while part p's table-gradient scatter (grid_bw, bound by memory-side atomics) keeps the memory
system busy.  n_parts = 1 is the plain single-batch step.

Buffers are sized once for the worst case (n_rays * MAX_SAMPLES samples, as the reference's
raymarching_train does); kernels that run per sample read the live count from their part's
`counter[0]` and grid-stride over it.  Parameters live in one flat fp32 vector
    params = [xyz MLP (3072) | rgb MLP (7168) | grid table (L*F*entries)]
so Adam is one launch and the gradient zeroing one memset; an fp16 mirror of the whole vector is
refreshed by the same Adam pass and is what the grid kernels gather from.
Multi-GPU: run/replay(exchange=dp.allreduce_mean_) all-reduces `grads` between backward and Adam.
HDR (StepConfig.hdr, the reference's --use_exposure): the field head returns log-radiance and the
three tonemappers sit between it and the compositing, forward and backward; their parameters are a
side group outside the flat vector with an Adam launch of their own (_tm_buffers, _tm_update).
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import synthetic
from ._lib import AdamFused, call, load, ptr, stream
from .field import XYZ_NET_PARAMS, rgb_net_params
from .grid import GridLayout

MAX_SAMPLES = 1024
GATE_TIMEOUT_US = 2000  # a gated march starts anyway after this long (gate.hip)
NEAR_DISTANCE = 0.01
SQRT3 = 3 ** 0.5
DENSITY_THRESHOLD = 0.01 * MAX_SAMPLES / SQRT3  # NGP.update_density_grid's threshold (train.py:165-168)
ADAM_BETAS = (0.9, 0.999)
POSE_ADAM_EPS = 1e-8
# synthetic scenes (scale <= 0.5) march with uniform steps over a white background; real scenes with
# exponentially growing steps over black, or a random colour (rendering.py:121-161)
EXP_STEP_FACTOR = 1 / 256
BG_SYNTHETIC, BG_REAL = 1.0, 0.0


@dataclass
class StepConfig:
    n_rays: int = 8192
    scale: float = 0.5
    L: int = 16
    F: int = 2
    log2_T: int = 19
    N_min: int = 16
    N_max: int = 2048
    grid: str = "Hash"
    N_tables: int = 1
    rgb_width: int = 64
    lr: float = 1e-2
    eps: float = 1e-15
    lambda_opacity: float = 1e-3
    lambda_distortion: float = 0.0  # NeRFLoss(lambda_distortion) = --distortion_loss_w (losses.py:40-60)
    T_threshold: float = 1e-4
    max_samples: int = MAX_SAMPLES
    n_parts: int = 1
    skip_nonfinite: bool = True  # GradScaler semantics: no optimizer step on an inf/nan gradient
    # PL precision=16 (train.py:287) = torch GradScaler defaults: init 2^16, x2 after 2000 clean steps,
    # x0.5 on an overflow; dynamic_loss_scale=False keeps a fixed 2^(floor(log2 n_rays)-2) instead
    dynamic_loss_scale: bool = True
    loss_scale: float = 65536.0
    growth_interval: int = 2000
    fixed_point_grid: bool = True  # table gradient by int32 fixed-point atomics (n_parts == 1)
    # ... of the hashed tables by partitioned LDS sums (mfnerf_grid_encode_bw_binned); False keeps the
    # memory-side-atomic scatter (the layouts the partitions do not support take it anyway)
    binned_grid: bool = True
    # the binned scatter's record slots are sized for this many samples per ray (the capacity is
    # max_samples = 1024 per ray; trained scenes march ~60): a step marching more than ~3x this
    # (the first steps, before the occupancy grid is pruned) overflows slots, whose extra records
    # are added by integer atomics (same sums, slower)
    bin_samples_per_ray: int = 128
    # the loss gradient with respect to the batch's rays (camera-pose refinement, train.py:91-94):
    # each part then carries dL_drays_o / dL_drays_d (Np,3), the unscaled gradient of the step's
    # loss, valid after run() and after a replay.  Off: the same launches as without the option
    ray_grads: bool = False
    # camera-pose refinement inside the step (train.py:91-94, 122-139, --optimize_ext): per-image
    # rotation / translation offsets trained by their own Adam (lr pose_lr) from the ray gradients,
    # the batch drawn from the refined poses.  Implies ray_grads; needs an attached dataset, one part,
    # no shard and no exchange.  Off: the same launches and buffers as without the option
    refine_poses: bool = False
    pose_lr: float = 1e-6
    # --random_bg (opt.py:49, rendering.py:153-161): on a real scene (scale > 0.5) the prediction is
    # blended over one random colour per training step -- every ray and every part of the step shares
    # it -- instead of black, so dark objects are not explained away as transparent; the target is
    # untouched.  The colour lives in the march buffer set of the batch it was drawn for (3 floats,
    # mbuf[j].bg): with an attached dataset the batch's own draw launch writes it, so a replayed step
    # reads the colour of the batch it trains on, not of the batch drawn ahead on the side stream.
    # Synthetic scenes (scale <= 0.5) ignore the flag: white, bit for bit the step without it.  Off:
    # the same launches and buffers as without the option
    random_bg: bool = False
    # --use_exposure, the HDR-NeRF model (train.py:73,102-103,172-177; networks.py:81-94,111-155): the
    # rgb head returns log-radiance (no sigmoid) and three tonemappers map log-radiance + log(exposure)
    # of the ray's image to the colour that is composited; the step's loss gains the unit-exposure
    # term 0.5 (tonemap(0, exposure 1) - unit_exposure_rgb)^2 (0.73 synthetic, 0.5 real: a property of
    # the dataset).  The tonemappers' 3 x 2048 parameters are a side group with their own Adam
    # (tm_params, tm_m, tm_v, tm_step_dev) sharing the field's lr, betas and eps.  Batches carry a
    # per-ray exposure (Batch.exposure, or the attached dataset's per-image exposures).  Needs one
    # part, no shard and no exchange.  Off: the same launches and buffers as without the option
    hdr: bool = False
    unit_exposure_rgb: float = 0.5

    def __post_init__(self):
        if self.refine_poses:
            self.ray_grads = True


@dataclass
class Batch:
    rays_o: torch.Tensor
    rays_d: torch.Tensor
    rgb: torch.Tensor
    buf: Optional[torch.Tensor] = None  # the (3, N, 3) buffer the three are views into, if packed
    exposure: Optional[torch.Tensor] = None  # (N,) f32 per-ray exposure (StepConfig.hdr)


class _State:
    @property
    def loss_sum(self):
        """The step's loss (device scalar): the sum of the loss partial sums."""
        return self.loss_parts.sum()


def _packed_batch(buf):
    """Batch whose tensors are views into one (3, N, 3) buffer (rays_o, rays_d, rgb)."""
    return Batch(buf[0], buf[1], buf[2], buf)


_nomark = lambda _name: None  # noqa: E731  (the mark= of a step nobody times)


TM_PARAMS = 2048  # one tonemapper (tonemap.N_PARAMS): W1 (64,16), then W2 (16,64), tcnn's layout


def init_params(c: StepConfig, n_params, n_alloc, seed):
    """The flat initial parameters [xyz MLP | rgb MLP | table] (host tensor, n_alloc long, zero
    padding): tcnn's init -- Xavier-uniform per MLP matrix, table U(-1e-4, 1e-4) -- from a seeded
    generator, so a CPU restatement of the step can start from the very same weights."""
    return _init_draws(c, n_params, n_alloc, seed)[0]


def init_tonemappers(c: StepConfig, n_params, n_alloc, seed):
    """The HDR step's initial tonemapper parameters (3, 2048), host tensor: tcnn's Xavier-uniform per
    matrix, drawn from init_params' generator AFTER its draws (the field's init is the LDR step's)."""
    return _draw_tonemappers(_init_draws(c, n_params, n_alloc, seed)[1])


def _draw_tonemappers(g):
    p = torch.zeros(3, TM_PARAMS)
    for ch in range(3):
        off = 0
        for o, k in [(64, 16), (16, 64)]:
            s = math.sqrt(6.0 / (o + k))
            p[ch, off:off + o * k].uniform_(-s, s, generator=g)
            off += o * k
    return p


def _init_draws(c: StepConfig, n_params, n_alloc, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(n_alloc)
    off = 0
    for o, k in [(64, 32), (16, 64), (c.rgb_width, 32), (c.rgb_width, c.rgb_width), (16, c.rgb_width)]:
        s = math.sqrt(6.0 / (o + k))  # tcnn Xavier-uniform per matrix
        p[off:off + o * k].uniform_(-s, s, generator=g)
        off += o * k
    p[off:n_params].uniform_(-1e-4, 1e-4, generator=g)  # tcnn grid init
    return p, g


class TrainStep:
    def __init__(self, cfg: StepConfig, device="cuda", seed=0):
        self.cfg = cfg
        self.dev = torch.device(device)
        load()
        c = cfg
        if c.n_parts < 1 or c.n_rays % c.n_parts:
            raise ValueError(f"n_rays={c.n_rays} must split into n_parts={c.n_parts} equal parts")
        if c.refine_poses and c.n_parts != 1:
            raise ValueError(f"refine_poses needs n_parts == 1 (got {c.n_parts}): the pose gradient is reduced "
                             "over the whole batch in one chain")
        if c.hdr and c.n_parts != 1:
            raise ValueError(f"hdr needs n_parts == 1 (got {c.n_parts}): the tonemappers' gradient is reduced "
                             "over the whole batch in one chain")
        self.cascades = max(1 + int(np.ceil(np.log2(2 * c.scale))), 1)
        self.G = 128
        b = float(np.exp(np.log(c.N_max * c.scale / c.N_min) / (c.L - 1)))
        self.layout = GridLayout(c.L, c.F, c.log2_T, c.N_min, b, c.grid, c.N_tables)
        self.desc = self.layout.desc()
        self.n_rgb = rgb_net_params(c.rgb_width)
        self.off_rgb = XYZ_NET_PARAMS
        self.off_table = XYZ_NET_PARAMS + self.n_rgb
        self.n_params = self.off_table + self.layout.n_params
        # flat buffers are padded (zeros, never updated) so any power-of-two world size shards them
        # into float4-aligned equal slices (shard_optimizer)
        self.n_alloc = -(-self.n_params // 16384) * 16384
        s32 = np.float32(c.scale)
        self.x_min, self.x_range = float(-s32), float(np.float32(s32) - np.float32(-s32))
        self.exp_step_factor, self.bg_value = (EXP_STEP_FACTOR, BG_REAL) if c.scale > 0.5 else (0.0, BG_SYNTHETIC)

        dev = self.dev
        p0, gen0 = _init_draws(c, self.n_params, self.n_alloc, seed)
        self.params = p0.to(dev)
        self.grads = torch.zeros(self.n_alloc, device=dev)
        self.m = torch.zeros(self.n_alloc, device=dev)
        self.v = torch.zeros(self.n_alloc, device=dev)
        self.p16 = self.params.half()
        self.shard = self.g_shard = None  # shard_optimizer(): (rank, lo, hi), this rank's slice of grads
        # mfnerf_amp_state: [non-finite flag, skipped steps, scale, growth tracker, growth interval,
        # growth factor, backoff factor, ticket] (include/mfnerf.h)
        self.finite_status = torch.zeros(8, dtype=torch.int32, device=dev)
        self.reset_loss_scale()
        self.packed = torch.empty(load().mfnerf_field_packed_bytes(c.rgb_width) // 2, dtype=torch.float16,
                                  device=dev)
        self._pack()
        self.adam_step = 0                                            # host mirror
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)  # Adam's t, bumped on the device
        self.lr_dev = torch.full((1,), float(c.lr), dtype=torch.float32, device=dev)
        # hdr: the tonemappers, a side parameter group (_tm_buffers); absent (None) without it
        self.tm_params = self.tm_grad = self.tm_m = self.tm_v = self.tm_step_dev = None
        if c.hdr:
            self._tm_buffers(_draw_tonemappers(gen0))
        del p0, gen0
        self.graphs = None
        self.samples_marched = torch.zeros(1, dtype=torch.int64, device=dev)

        # scene bounding box (networks.py:18-23) and occupancy
        self.center = torch.zeros(1, 3, device=dev)
        self.half_size = torch.full((1, 3), c.scale, device=dev)
        self.density_grid = torch.zeros(self.cascades, self.G ** 3, device=dev)
        self.bitfield = torch.zeros(self.cascades * self.G ** 3 // 8, dtype=torch.uint8, device=dev)

        N = c.n_rays
        self.n_parts = c.n_parts
        self.Np = N // c.n_parts                      # rays per part
        self.cap_p = self.Np * c.max_samples          # sample capacity per part
        self.cap = N * c.max_samples
        self._bin_supported = (c.n_parts == 1 and c.fixed_point_grid and c.binned_grid and
                               load().mfnerf_grid_encode_bw_binned_workspace(self.desc, self._bin_slots()) >= 0)
        self._store_fold_v = self._store_fold()
        self._fused_args = None  # the last mfnerf_adam_fused handed to a launch, kept alive for the graphs
        self.parts = [self._part_buffers(q) for q in range(c.n_parts)]
        self._bg_const = torch.full((3,), self.bg_value, dtype=torch.float32, device=dev)
        # attach_dataset: the dataset, the batch drawn from it (and, refine_poses only, _pose_buffers)
        self.dataset = self._sampled = None
        self.mbuf = [self._march_buffers()]  # a second set is added by capture() (pipelined march)
        # the step's loss as partial sums: one per 4 rays of each part (written by the fused
        # compositing kernel) + 64 accumulated slots (unfused path: NeRFLoss atomics, distortion)
        self._nb_part = -(-self.Np // 4)
        self._level_l1 = torch.zeros(c.L, dtype=torch.float32, device=dev)
        # (+ hdr: the unit-exposure term's three channel shares, stored by mfnerf_tonemap_unit_loss)
        n_fused = c.n_parts * self._nb_part
        self.loss_parts = torch.zeros(n_fused + 64 + (3 if c.hdr else 0), dtype=torch.float32, device=dev)
        self._loss_acc = self.loss_parts[n_fused:n_fused + 64]
        self._loss_unit = self.loss_parts[n_fused + 64:]
        self.state = _State()
        self._use(self.mbuf[0])
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed + 1)
        # static fp16 backward scale: per-sample grads are O(1/n_rays); 2^(floor(log2 N)-2) keeps them
        # normal.  With the dynamic scale (default) field_bw reads amp.scale on the device instead.
        self.grad_scale = float(2.0 ** max(0, int(math.floor(math.log2(N))) - 2))
        self.last_batch = None    # the batch of the last step (run: as passed or drawn; replay: the static set)
        self._stale_pack = False  # a one-graph data-parallel replay left `packed` one update behind
        self._occ = None          # the occupancy refresh's scratch and graphs (_occ_buffers)
        # what capture() makes: static inputs per march buffer set, the device gate of the gated march
        # ({signals, waits, -, timeouts}; None: the captured step is not gated), streams and events
        self._static, self._static_noise, self._static_bg, self._host_noise = [], None, None, False
        self._gate, self._gate_opened, self._side, self._part_streams = None, 0, None, []
        self._ev_start, self._ev_march, self._ev_chain, self._ev_part = None, [], [], []
        self._parity = 0      # the march buffer set of the next replay
        self._primed = False  # ... whose batch is already marched (by the previous replay)

    def reset_loss_scale(self, scale=None):
        """(Re)initialise the device GradScaler state (mfnerf_amp_state) from the config."""
        c = self.cfg
        a = torch.zeros(8, dtype=torch.int32)
        af = a.view(torch.float32)
        af[2] = float(c.loss_scale if scale is None else scale)
        a[4] = int(c.growth_interval) if c.dynamic_loss_scale else 0
        af[5], af[6] = 2.0, 0.5
        self.finite_status.copy_(a.to(self.dev))

    def _amp_on(self):
        """GradScaler bookkeeping on the device: the skip (and, dynamic, the scale update)."""
        return self.cfg.skip_nonfinite or self.cfg.dynamic_loss_scale

    def _amp_ptr(self):
        return ptr(self.finite_status) if self._amp_on() else None

    def loss_scale(self):
        """The loss scale the next backward uses (host read)."""
        if not self.cfg.dynamic_loss_scale:
            return self.grad_scale
        return float(self.finite_status.view(torch.float32)[2])

    def attach_dataset(self, ds):
        """Draw every step's batch on the device from ds (mfnerf.data.DeviceDataset): run() and
        replay() then take no batch; inside graphs the draw is part of the march graph."""
        self.dataset = ds
        self._sampled = _packed_batch(torch.zeros(3, self.cfg.n_rays, 3, device=self.dev))
        self.graphs = None
        if self.cfg.refine_poses:
            self._pose_buffers(ds)

    # ---------------------------------------------------------------- HDR / exposure
    def _tm_buffers(self, p0):
        """The tonemappers as a side parameter group (as dR / dT are): parameters, the step's gradient,
        Adam moments and step count, all touched on the main stream only."""
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.tm_params = p0.to(self.dev).contiguous()
        self.tm_grad = torch.zeros(3, TM_PARAMS, **f32)
        self.tm_m = torch.zeros(3, TM_PARAMS, **f32)
        self.tm_v = torch.zeros(3, TM_PARAMS, **f32)
        self.tm_step_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def _check_hdr(self, exchange=None):
        if not self.cfg.hdr:
            return
        if self.shard is not None or exchange is not None:
            raise ValueError("hdr does not run with a sharded optimizer or a gradient exchange: "
                             "data-parallel HDR training is out of scope")
        if self.dataset is not None and self.dataset.exposure is None:
            raise ValueError("hdr needs a dataset with per-image exposures (DeviceDataset(exposure=...))")

    def _stage_exposure(self, batch, mb):
        """A passed batch's per-ray exposure into the march buffer set the batch is marched into."""
        e = batch.exposure
        if e is None:
            raise ValueError("hdr: a batch the caller passes needs its per-ray exposure (Batch.exposure, (N,) f32)")
        if e.numel() != self.cfg.n_rays:
            raise ValueError(f"hdr: Batch.exposure has {e.numel()} values for {self.cfg.n_rays} rays")
        mb.exposure.copy_(e.reshape(-1))

    def _tonemap_fw(self, mb, q):
        """rendering.py:142-145 + networks.py:111-132 between the field and the compositing: the rays'
        exposures repeated per sample, then log-radiance + log(exposure) through the tonemappers into
        rgb_s (fp32 holding the half values, what the compositing reads)."""
        t, m, cap, s = self.parts[q], mb.part[q], self.cap_p, stream()
        call("mfnerf_expand_exposure", ptr(mb.exposure[q * self.Np:(q + 1) * self.Np]), ptr(m.rays_a), self.Np, cap,
             ptr(m.counter), ptr(t.exposure_s), s)
        call("mfnerf_tonemap_fw_live", ptr(t.lograd), ptr(t.exposure_s), 1, cap, ptr(m.counter), ptr(self.tm_params),
             ptr(t.rgb_s), s)

    def _tonemap_bw(self, mb, q):
        """dL/drgb_s -> dL/dlograd and the tonemappers' gradient (overwritten), then the unit-exposure
        term (train.py:172-177): its loss into the step's loss slots, its gradient added on top; a
        non-finite tonemapper gradient raises the step's flag."""
        t, m, cap, s = self.parts[q], mb.part[q], self.cap_p, stream()
        call("mfnerf_tonemap_bw_live", ptr(t.lograd), ptr(t.exposure_s), 1, cap, ptr(m.counter), ptr(self.tm_params),
             ptr(t.rgb_s), ptr(t.drgb_s), ptr(t.dlograd), ptr(self.tm_grad), ptr(t.tm_ws), s)
        call("mfnerf_tonemap_unit_loss", ptr(self.tm_params), 3, float(self.cfg.unit_exposure_rgb), ptr(self.tm_grad),
             ptr(self._loss_unit), self._amp_ptr(), s)

    def _tm_update(self):
        """The tonemappers' Adam (train.py:131-136: the field's lr, betas and eps), after field_bw -- the
        step's non-finite flag is final -- and before the main optimizer call, which clears it: a
        skipped step skips both."""
        call("mfnerf_side_adam_step", ptr(self.tm_params), ptr(self.tm_grad), ptr(self.tm_m), ptr(self.tm_v),
             self.tm_params.numel(), float(self.cfg.lr), *ADAM_BETAS, self.cfg.eps, ptr(self.tm_step_dev),
             ptr(self.lr_dev), self._amp_ptr(), stream())

    # ---------------------------------------------------------------- pose refinement
    def _pose_buffers(self, ds):
        """The pose state (train.py:122-128: dR, dT zero) and its Adam moments, touched only on the
        main stream, and one refined-pose buffer per march buffer set: the draw into set j reads
        pose_buf[j], the step that trains on set j writes its updated composition back into it -- the
        draw that read it is long done, the next one is two steps away and ordered by the replay's
        events.  The next step's draw, which runs beside this step, reads the other buffer, so it never
        reads what this step writes (and sees the updates one step late)."""
        dev, n = self.dev, ds.n_img
        f32 = dict(dtype=torch.float32, device=dev)
        self.dR = torch.zeros(n, 3, **f32)
        self.dT = torch.zeros(n, 3, **f32)
        self.pose_m = torch.zeros(2, n, 3, **f32)
        self.pose_v = torch.zeros(2, n, 3, **f32)
        self.pose_grad = torch.zeros(2, n, 3, **f32)  # grad_dR | grad_dT of the last step
        self.pose_step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pose_lr_dev = torch.full((1,), float(self.cfg.pose_lr), **f32)
        self.pose_buf = [ds.poses.clone(), ds.poses.clone()]
        for mb in self.mbuf:
            self._pose_idx_buffers(mb)

    def _pose_idx_buffers(self, mb):
        mb.img_idx = torch.zeros(self.cfg.n_rays, dtype=torch.int32, device=self.dev)
        mb.pix_idx = torch.zeros(self.cfg.n_rays, dtype=torch.int32, device=self.dev)

    def _check_refine(self, exchange=None):
        if not self.cfg.refine_poses:
            return
        if self.dataset is None:
            raise ValueError("refine_poses needs an attached dataset (attach_dataset): the step draws its batch "
                             "from the refined poses")
        if self.shard is not None or exchange is not None:
            raise ValueError("refine_poses does not run with a sharded optimizer or a gradient exchange: "
                             "data-parallel pose refinement is out of scope")

    def set_pose_lr(self, lr):
        """The pose optimizer's device-resident learning rate."""
        self.pose_lr_dev.fill_(float(lr))

    def compose_poses(self):
        """Both refined-pose buffers from the current dR / dT (no update).  Call with the side stream
        idle (capture() and a checkpoint load do)."""
        for buf in self.pose_buf:
            call("mfnerf_pose_step", ptr(self.dR), ptr(self.dT), None, None, None, None, ptr(self.dataset.poses),
                 self.dataset.n_img, 0.0, *ADAM_BETAS, POSE_ADAM_EPS, None, None, None, ptr(buf), stream())

    def _pose_update(self, mb):
        """After the ray gradients of the step on mb: the per-image reduction, the pose Adam step (skipped
        with the field's on a non-finite gradient) and the refined poses into mb's pose buffer."""
        ds, t = self.dataset, self.parts[0]
        call("mfnerf_pose_grad", ptr(t.dL_drays_o), ptr(t.dL_drays_d), ptr(mb.img_idx), ptr(mb.pix_idx),
             ptr(ds.poses), ptr(ds.directions), ptr(self.dR), self.cfg.n_rays, ds.n_img, ds.hw,
             ptr(self.pose_grad[0]), ptr(self.pose_grad[1]), self._amp_ptr(), stream())
        call("mfnerf_pose_step", ptr(self.dR), ptr(self.dT), ptr(self.pose_m), ptr(self.pose_v),
             ptr(self.pose_grad[0]), ptr(self.pose_grad[1]), ptr(ds.poses), ds.n_img, float(self.cfg.pose_lr),
             *ADAM_BETAS, POSE_ADAM_EPS, ptr(self.pose_step_dev), ptr(self.pose_lr_dev), self._amp_ptr(),
             ptr(self.pose_buf[self.mbuf.index(mb)]), stream())

    # ---------------------------------------------------------------- buffers
    def _part_buffers(self, q):
        """Per-part sample/ray state of the chain (features, field outputs, compositing, grads)."""
        c, dev, Np, cap = self.cfg, self.dev, self.Np, self.cap_p
        f32 = dict(dtype=torch.float32, device=dev)
        t = _State()
        # encoded features as level planes (L, cap) of half2 (mfnerf_grid_encode_fw_planar)
        t.feat = torch.empty(c.L, cap, c.F, dtype=torch.float16, device=dev)
        t.sigma = torch.empty(cap, **f32)
        t.rgb_s = torch.empty(cap, 3, **f32)
        t.total = torch.empty(Np, dtype=torch.int64, device=dev)
        t.opacity = torch.empty(Np, **f32)
        t.depth = torch.empty(Np, **f32)
        t.rgb = torch.empty(Np, 3, **f32)
        t.ws = torch.empty(cap, **f32)
        t.dL_drgb = torch.empty(Np, 3, **f32)
        t.dL_dop = torch.empty(Np, **f32)
        t.zeros_ray = torch.zeros(Np, **f32)       # dL/ddepth (unused by the loss; unfused path)
        if c.lambda_distortion > 0:                # losses.py:6-37 + 55-58
            t.dist_loss = torch.empty(Np, **f32)
            t.ws_incl = torch.empty(cap, **f32)
            t.wts_incl = torch.empty(cap, **f32)
            t.dL_ddist = torch.full((Np,), c.lambda_distortion / c.n_rays, **f32)  # d(lambda*mean)/dloss_r
            t.dL_dws = torch.empty(cap, **f32)
        t.dsig = torch.empty(cap, **f32)
        t.drgb_s = torch.empty(cap, 3, **f32)
        t.dfeat = torch.empty(cap, c.L * c.F, **f32)
        t.field_ws = torch.empty(load().mfnerf_field_bw_workspace(cap, c.rgb_width) // 4, **f32)
        if c.ray_grads:
            t.ddirs = torch.empty(cap, 3, **f32)
            t.dL_drays_o = torch.zeros(Np, 3, **f32)
            t.dL_drays_d = torch.zeros(Np, 3, **f32)
        if c.hdr:
            t.lograd = torch.empty(cap, 3, dtype=torch.float16, device=dev)  # the head's fp16 output
            t.exposure_s = torch.empty(cap, **f32)
            t.dlograd = torch.empty(cap, 3, **f32)
            t.tm_ws = torch.empty(max(16, load().mfnerf_tonemap_bw_workspace(cap, 3)) // 4, **f32)
        nb = (load().mfnerf_grid_encode_bw_binned_workspace(self.desc, self._bin_slots()) if self._binned()
              else load().mfnerf_grid_encode_bw_workspace(self.desc))
        t.grid_ws = torch.zeros(max(16, nb) // 4, **f32)
        # parts > 0 accumulate their MLP weight grads privately (field_bw's slab sum is a plain +=)
        t.mlp_grad = self.grads[:self.off_table] if q == 0 else torch.zeros(self.off_table, **f32)
        return t

    def _march_buffers(self):
        """One set of ray-march outputs: AABB hits and noise for the whole batch, samples per part."""
        c, N, dev = self.cfg, self.cfg.n_rays, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        m = _State()
        m.hit_cnt = torch.empty(N, dtype=torch.int32, device=dev)
        m.hits = torch.empty(N, 1, 2, **f32)
        m.hits_t = m.hits[:, 0]
        m.hits_idx = torch.empty(N, 1, dtype=torch.int64, device=dev)
        m.noise = torch.empty(N, **f32)
        m.counters = torch.zeros(c.n_parts, 2, dtype=torch.int32, device=dev)  # per part (samples, rays)
        m.part = []
        for q in range(c.n_parts):
            t = _State()
            t.rays_a = torch.empty(self.Np, 3, dtype=torch.int64, device=dev)
            t.xyzs = torch.empty(self.cap_p, 3, **f32)
            t.dirs = torch.empty(self.cap_p, 3, **f32)
            t.deltas = torch.empty(self.cap_p, **f32)
            t.ts = torch.empty(self.cap_p, **f32)
            t.counter = m.counters[q]
            ws_bytes = load().mfnerf_raymarching_train_workspace(self.Np, c.max_samples)
            t.march_ws = torch.empty(max(16, ws_bytes), dtype=torch.uint8, device=dev)
            m.part.append(t)
        if c.hdr or (c.refine_poses and self.dataset is not None):
            self._pose_idx_buffers(m)
        if c.hdr:
            m.exposure = torch.ones(N, **f32)  # per ray, of the batch marched into this set
        if self._random_bg():
            m.bg = torch.zeros(3, **f32)  # the colour of the batch marched into this set
        return m

    def _random_bg(self):
        """random_bg in effect: the reference draws a colour only when exp_step_factor != 0
        (rendering.py:153-161), here scale > 0.5."""
        return self.cfg.random_bg and self.cfg.scale > 0.5

    def _use(self, mb):
        """state.noise / state.counters / state.loss_sum / state.bg of the step being run (inspection)."""
        st = self.state
        st.noise, st.counters, st.loss_parts, st.march = mb.noise, mb.counters, self.loss_parts, mb
        st.parts = self.parts
        st.bg = mb.bg if self._random_bg() else self._bg_const

    @property
    def bg(self):
        """The background colour (device 3-vector) the last step trained with: with random_bg on a real
        scene the colour of that step's batch, else the constant white (synthetic) or black vector."""
        return self.state.bg

    @property
    def loss_sum(self):
        return self.loss_parts.sum()

    def live_samples(self):
        """Device scalar: samples marched by the current step (sum over parts)."""
        return self.state.counters[:, 0].sum()

    def gather_march(self):
        """(rays_a (N,3) i64 with global starts, xyzs (n,3), dirs, deltas, ts) of the current step,
        concatenated over parts in ray order -- host-synchronising, for tests and smoke()."""
        mb = self.state.march
        ra, xs, ds, dl, ts = [], [], [], [], []
        base = 0
        for q, t in enumerate(mb.part):
            n = int(mb.counters[q, 0])
            r = t.rays_a.clone()
            r[:, 0] += q * self.Np
            r[:, 1] += base
            ra.append(r)
            xs.append(t.xyzs[:n]); ds.append(t.dirs[:n]); dl.append(t.deltas[:n]); ts.append(t.ts[:n])
            base += n
        return torch.cat(ra), torch.cat(xs), torch.cat(ds), torch.cat(dl), torch.cat(ts)

    # ---------------------------------------------------------------- data
    def make_batches(self, k, seed=0):
        """k synthetic Lego-like ray batches (mfnerf.synthetic), resident on the device; each is
        packed in one (3, N, 3) buffer (rays_o, rays_d, rgb) so replay() refreshes with one copy."""
        poses = synthetic.camera_poses(seed=seed)
        out = []
        for i in range(k):
            o, d = synthetic.random_rays(self.cfg.n_rays, poses, seed=seed * 1000 + i)
            dn = d / d.norm(dim=1, keepdim=True)
            gt = 0.5 + 0.5 * torch.sin(3 * dn + torch.tensor([0.0, 1.0, 2.0]))  # smooth view-dependent target
            out.append(_packed_batch(torch.stack([o, d, gt.float()]).to(self.dev)))
        return out

    def set_occupancy(self, density_grid):
        """Install a (C, G^3) density grid and pack it with the reference's threshold."""
        self.density_grid.copy_(density_grid.to(self.dev))
        call("mfnerf_packbits", ptr(self.density_grid), self.bitfield.numel(), DENSITY_THRESHOLD, None,
             ptr(self.bitfield), stream())

    def _pack(self):
        """MFMA weight blob from the fp16 compute copy (the fp16 values packing the fp32 master
        would produce), so it works on every rank when the fp32 master is sharded."""
        call("mfnerf_field_pack_weights_f16", ptr(self.p16), ptr(self.p16[self.off_rgb:]), self.cfg.rgb_width,
             ptr(self.packed), stream())

    def _flush_pack(self):
        """Repack if a one-graph data-parallel replay deferred it: that path's Adam runs after the
        collective and the next dp_pre graph starts with the repack, so until then `packed` is one
        update behind.  Everything else that reads `packed` (an eager step, the occupancy refresh,
        the per-stage graphs) calls this first."""
        if self._stale_pack:
            pg = (self.graphs or {}).get("pack")
            pg.replay() if pg is not None else self._pack()
            self._stale_pack = False

    def shard_optimizer(self, rank, world, force=False):
        """Data parallel with a sharded optimizer (mfnerf.dp.sharded_update): this rank keeps Adam
        state only for its 1/world slice of the flat parameters; the step reduce-scatters the
        gradient, updates the slice and all-gathers the fp16 compute copy.  world 1 is a no-op
        unless force (a one-rank process group running the sharded path, for tests)."""
        if world <= 1 and not force:
            return
        if self.cfg.refine_poses:
            raise ValueError("refine_poses does not run with a sharded optimizer: data-parallel pose refinement "
                             "is out of scope")
        if self.cfg.hdr:
            raise ValueError("hdr does not run with a sharded optimizer: data-parallel HDR training is out of scope")
        if self.n_alloc % (64 * world):
            raise ValueError(f"world size {world} does not divide the padded parameter count {self.n_alloc}")
        k = self.n_alloc // world
        lo, hi = rank * k, (rank + 1) * k
        self.shard = (rank, lo, hi)
        self.m = torch.zeros(k, device=self.dev)
        self.v = torch.zeros(k, device=self.dev)
        # this rank's slice of the gradient, reduced in place (RCCL in-place reduce-scatter: no
        # second gradient-sized buffer, and a one-rank group's "reduction" is no copy)
        self.g_shard = self.grads[lo:hi]
        self._store_fold_v = self._store_fold()
        self.graphs = None  # re-capture with the sharded update

    # ---------------------------------------------------------------- the step
    def _draw(self, batch: Batch, mb):
        """The attached dataset's next batch into `batch`, with the march prologue (AABB + near clamp
        + noise) of mb in the same launch -- and, random_bg, the batch's background colour into mb.bg."""
        prep = (self.center, self.half_size, NEAR_DISTANCE, mb.hits, mb.noise)
        kw = {"bg": mb.bg} if self._random_bg() else {}
        if self.cfg.refine_poses:
            kw.update(img_idx=mb.img_idx, pix_idx=mb.pix_idx, poses=self.pose_buf[self.mbuf.index(mb)])
        if self.cfg.hdr:
            kw.update(img_idx=mb.img_idx, pix_idx=mb.pix_idx)
        self.dataset.sample(batch.buf, prep=prep, **kw)
        if self.cfg.hdr:  # datasets/base.py:34-35: a ray's exposure is its image's (a gather on the draw's stream)
            torch.index_select(self.dataset.exposure, 0, mb.img_idx, out=mb.exposure)

    def _march(self, batch: Batch, mb, mark, prepped=False, noise=None, bg=None):
        """AABB + near clamp + noise (and, random_bg, the background colour: from the step's generator
        after the noise, or the given bg) for the whole batch (unless _draw did it), then one ray march
        per part into mb."""
        c, s = self.cfg, stream()
        N, Np = c.n_rays, self.Np
        if not prepped:
            # rendering.py:27-29 (AABB + near clamp), custom_functions.py:83 (noise)
            call("mfnerf_ray_aabb_intersect", ptr(batch.rays_o), ptr(batch.rays_d), ptr(self.center),
                 ptr(self.half_size), N, 1, 1, ptr(mb.hit_cnt), ptr(mb.hits), ptr(mb.hits_idx), s)
            t1 = mb.hits[:, 0, 0]
            t1.masked_fill_((t1 >= 0) & (t1 < NEAR_DISTANCE), NEAR_DISTANCE)
            if noise is None:
                torch.rand(N, generator=self.gen, device=self.dev, out=mb.noise)
            else:  # a given perturbation (parity tests driving the reference with the same draws)
                mb.noise.copy_(noise)
            if self._random_bg():  # rendering.py:160: one colour for the whole batch
                if bg is None:
                    torch.rand(3, generator=self.gen, device=self.dev, out=mb.bg)
                else:
                    mb.bg.copy_(torch.as_tensor(bg, dtype=torch.float32).reshape(3))
        mark("prep")
        for q, t in enumerate(mb.part):
            r = slice(q * Np, (q + 1) * Np)
            call("mfnerf_raymarching_train", ptr(batch.rays_o[r]), ptr(batch.rays_d[r]), ptr(mb.hits_t[r]), 2,
                 ptr(self.bitfield), self.cascades, float(c.scale), self.exp_step_factor, ptr(mb.noise[r]), self.G,
                 c.max_samples, Np, self.cap_p, ptr(t.rays_a), ptr(t.xyzs), ptr(t.dirs), ptr(t.deltas), ptr(t.ts),
                 ptr(t.counter), ptr(t.march_ws), s)
        # running total of marched samples (rm_s without a read on the step's critical path: in the
        # graphs this runs on the march's side stream): one kernel for one part, else slice + reduce + add
        self.samples_marched.add_(mb.counters[0, 0] if self.n_parts == 1 else mb.counters[:, 0].sum())
        mark("march")

    def _enc_args(self, mb, q):
        """The encoding's forward and every scatter start with: part q's samples in mb, their count, box, grid."""
        m = mb.part[q]
        return ptr(m.xyzs), self.cap_p, ptr(m.counter), self.x_min, self.x_range, self.desc

    def _chain(self, batch: Batch, mb, q, mark, side_adam=True):
        """Part q: encode -> field -> composite -> loss -> composite bw -> field bw (no grid bw).
        Part 0 also zeroes the gradient (every part's writes come after it).  hdr: the field head
        without its sigmoid, the tonemappers between it and the compositing in both directions, the
        unit-exposure term, and (side_adam) the tonemappers' Adam at the end."""
        c, s = self.cfg, stream()
        t, m = self.parts[q], mb.part[q]
        Np, cap = self.Np, self.cap_p
        store_fold = q == 0 and self._store_fold_v
        if q == 0:
            if self.shard is not None and not store_fold:
                # unsharded: the previous Adam pass left it zero; sharded, the binned scatter
                # overwrites the partitioned tables, so only the values before them are zeroed
                self.grads[:self._grad_zero_end()].zero_()
            if c.lambda_distortion > 0:
                self._loss_acc.zero_()
        else:
            t.mlp_grad.zero_()
        call("mfnerf_grid_encode_fw_planar", *self._enc_args(mb, q), ptr(self.p16[self.off_table:]), ptr(t.feat),
             cap, s)
        mark("grid_fw")
        if c.hdr:
            call("mfnerf_field_fw_lograd", ptr(t.feat), cap, ptr(m.dirs), cap, ptr(m.counter), ptr(self.packed),
                 c.rgb_width, ptr(t.sigma), ptr(t.lograd), s)
            mark("field_fw")
            self._tonemap_fw(mb, q)
            mark("tonemap_fw")
        else:
            call("mfnerf_field_fw", ptr(t.feat), cap, ptr(m.dirs), cap, ptr(m.counter), ptr(self.packed), c.rgb_width,
                 0, ptr(t.sigma), ptr(t.rgb_s), s)
            mark("field_fw")
        # the background: three scalars, or (random_bg) the 3 floats the batch's draw left in mb.bg,
        # read by the _bg forms of the two loss-carrying kernels (every part reads the one colour)
        bg = self.bg_value
        sfx, bg_args = ("_bg", (ptr(mb.bg),)) if self._random_bg() else ("", (bg, bg, bg))
        target = ptr(batch.rgb[q * Np:(q + 1) * Np])
        comp_in = (ptr(t.sigma), ptr(t.rgb_s), ptr(m.deltas), ptr(m.ts), ptr(m.rays_a), Np, cap, c.T_threshold)
        comp_out = (ptr(t.total), ptr(t.opacity), ptr(t.depth), ptr(t.rgb), ptr(t.ws))
        if c.lambda_distortion <= 0:
            # composite fw -> bg blend + NeRFLoss -> composite bw in one wave-per-ray launch
            call("mfnerf_composite_train_fused" + sfx, *comp_in, target, c.n_rays, c.lambda_opacity, *bg_args,
                 *comp_out, ptr(t.dL_drgb), ptr(t.dL_dop), ptr(t.dsig), ptr(t.drgb_s),
                 ptr(self.loss_parts[q * self._nb_part:]), s)
            mark("composite")
        else:
            call("mfnerf_composite_train_fw", *comp_in, *comp_out, s)
            call("mfnerf_nerf_loss" + sfx, ptr(t.rgb), ptr(t.opacity), target, Np, c.n_rays, c.lambda_opacity,
                 *bg_args, ptr(t.dL_drgb), ptr(t.dL_dop), ptr(self._loss_acc), s)
            # losses.py:6-37 + 55-58
            call("mfnerf_distortion_loss_fw", ptr(t.ws), ptr(m.deltas), ptr(m.ts), ptr(m.rays_a), Np, cap,
                 ptr(t.dist_loss), ptr(t.ws_incl), ptr(t.wts_incl), s)
            self._loss_acc[1:2].add_(t.dist_loss.sum() * (c.lambda_distortion / c.n_rays))
            call("mfnerf_distortion_loss_bw", ptr(t.dL_ddist), ptr(t.ws_incl), ptr(t.wts_incl), ptr(t.ws),
                 ptr(m.deltas), ptr(m.ts), ptr(m.rays_a), Np, cap, ptr(t.dL_dws), s)
            mark("composite_fw")
            call("mfnerf_composite_train_bw", ptr(t.dL_dop), ptr(t.zeros_ray), ptr(t.dL_drgb), ptr(t.dL_dws),
                 ptr(t.sigma), ptr(t.rgb_s), ptr(t.ws), ptr(m.deltas), ptr(m.ts), ptr(m.rays_a), ptr(t.opacity),
                 ptr(t.depth), ptr(t.rgb), Np, cap, c.T_threshold, ptr(t.dsig), ptr(t.drgb_s), s)
            mark("composite_bw")
        lograd = ""
        if c.hdr:
            self._tonemap_bw(mb, q)
            mark("tonemap_bw")
            lograd = "_lograd"  # the head's output gradient is dL/dlograd, no y(1-y)
        bw_args = (ptr(t.feat), cap, ptr(m.dirs), cap, ptr(m.counter), ptr(self.packed), c.rgb_width,
                   ptr(t.dsig), ptr(t.dlograd if c.hdr else t.drgb_s),
                   0.0 if c.dynamic_loss_scale else self.grad_scale, ptr(t.dfeat),
                   None if store_fold else ptr(t.mlp_grad), None if store_fold else ptr(t.mlp_grad[self.off_rgb:]),
                   ptr(t.field_ws), self._amp_ptr(), ptr(self._level_l1) if self._fixed() else None)
        if c.ray_grads:
            # the same backward plus dL/ddirs, then dL/dxyz through the encoding summed per ray
            # (the table is the fp16 copy the forward gathered from: Adam comes later in the step)
            call("mfnerf_field_bw_inputs" + lograd, *bw_args, ptr(t.ddirs), s)
            call("mfnerf_rays_input_grad", ptr(m.xyzs), ptr(m.ts), ptr(t.dfeat), ptr(t.ddirs), ptr(m.rays_a), Np, cap,
                 self.x_min, self.x_range, self.desc, ptr(self.p16[self.off_table:]), ptr(t.dL_drays_o),
                 ptr(t.dL_drays_d), s)
        else:
            call("mfnerf_field_bw" + lograd, *bw_args, s)
        if store_fold:  # the fold writes the MLPs' gradient outright (nothing zeroed it)
            call("mfnerf_field_bw_reduce_store", c.rgb_width, ptr(t.field_ws), ptr(t.mlp_grad),
                 ptr(t.mlp_grad[self.off_rgb:]), self._amp_ptr(), s)
        if c.refine_poses:
            self._pose_update(mb)
        if c.hdr and side_adam:
            self._tm_update()
        mark("field_bw")

    def _fixed(self):
        """One part: the table gradient is accumulated by int32 fixed-point atomics (per-level scales
        bounded by the L1 norm of dL/dfeat, which field_bw accumulates, so no overflow; the table
        gradient starts at zero because Adam zeroed it); several parts share the gradient and use
        float atomics."""
        return self.n_parts == 1 and self.cfg.fixed_point_grid

    def _binned(self):
        """The fixed-point table gradient by table partitions (one part only, like _fixed), for the
        layouts the partitioned scatter supports; any other layout the reference accepts (opt.py:78,
        e.g. --T 21) keeps the request-shaped fixed-point atomic scatter."""
        return self._bin_supported

    def _bin_slots(self):
        """Samples per part the binned scatter's record slots are sized for."""
        return min(self.cap_p, self.Np * max(1, self.cfg.bin_samples_per_ray))

    def _fused_adam_ok(self):
        """The collective-free replayed tail can run the partitioned tables' Adam inside the scatter's
        accumulate (mfnerf_grid_encode_bw_binned_adam + mfnerf_adam_step_fixed_partial)."""
        return self._binned() and self.shard is None and load().mfnerf_grid_binned_first_value(self.desc) >= 0

    def _adam_args(self):
        """Every Adam entry point's (lr, beta1, beta2, eps), (device step count, device lr, GradScaler state)."""
        return (float(self.cfg.lr), *ADAM_BETAS, self.cfg.eps), (ptr(self.step_dev), ptr(self.lr_dev), self._amp_ptr())

    def _open_gate(self, gate, in_launch):
        """A scatter opens the side stream's gate as it starts: its dense-level launch's first workgroup
        (in_launch: the entry point takes the pointer), else a signal kernel just before it.  Counted."""
        if gate is not None:
            self._gate_opened += 1
            if not in_launch:
                call("mfnerf_gate_signal", gate, stream())

    def _scatter_args(self, mb, q):
        """(samples, count, box, grid, dL/dfeat), table gradient, the binned forms' (workspace, slots, level_l1)."""
        t = self.parts[q]
        return ((*self._enc_args(mb, q), ptr(t.dfeat)), ptr(self.grads[self.off_table:]),
                (ptr(t.grid_ws), self._bin_slots(), ptr(self._level_l1)))

    def _grid_bw(self, mb, q, fuse_adam=False, gate=None):
        """Part q's hash-table gradient scatter (the dominant kernel, alone so it can be timed);
        fuse_adam: with the partitioned tables' Adam step (then _finish_update(partial=True));
        fuse_adam="all": with the whole optimizer step and the MLP repack.  gate: see _open_gate."""
        src, table, (ws, slots, l1) = self._scatter_args(mb, q)
        binned = self._binned()
        fuse_all = binned and fuse_adam == "all"
        self._open_gate(gate, in_launch=fuse_all)
        if binned and fuse_adam:
            (lr, beta1, beta2, eps), (step_dev, lr_dev, amp) = self._adam_args()
            self._fused_args = AdamFused(  # kept alive: graphs capture the call
                params=self.params.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), p16=self.p16.data_ptr(),
                table_offset=self.off_table, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step_dev=step_dev.value,
                lr_dev=lr_dev.value, amp=amp.value if amp is not None else None)
        if fuse_all:
            call("mfnerf_grid_encode_bw_binned_adam_all", *src, ptr(self.grads), self.n_alloc, ws, slots, l1,
                 ctypes.byref(self._fused_args), ptr(self.step_dev), self._amp_ptr(), ptr(self.packed),
                 self.cfg.rgb_width, gate, stream())
        elif binned and fuse_adam:
            call("mfnerf_grid_encode_bw_binned_adam", *src, table, ws, slots, l1, ctypes.byref(self._fused_args),
                 stream())
        elif binned:
            # both parts in sequence on this stream: the coarse levels' atomics, then the fine levels'
            # partitioned sums (the two on separate streams inside the graphs measured 1.32 vs
            # 0.87 ms per step: the extra branch slowed every kernel beside it)
            call("mfnerf_grid_encode_bw_binned", *src, table, ws, slots, l1, 3, stream())
        else:
            call("mfnerf_grid_encode_bw_scatter", *src, table, ws, l1 if self._fixed() else None, stream())

    def _store_fold(self):
        """Sharded, one part, partitioned scatter whose float finish overwrites every table value
        before the partitioned tables (they are all dense-prefix values): the weight-gradient fold
        stores instead of adding and the step zeroes no gradient prefix (one fill launch less).
        Evaluated once per sharding: _store_fold_v."""
        lib, w = load(), self.cfg.rgb_width
        n_dw = lib.mfnerf_field_bw_workspace(0, w) // (4 * lib.mfnerf_field_bw_slab_rows(w))
        return (self.shard is not None and self.n_parts == 1 and self._binned() and self._fixed()
                and self.off_table == n_dw
                and lib.mfnerf_grid_binned_first_value(self.desc) == lib.mfnerf_grid_dense_values(self.desc))

    def _grad_zero_end(self):
        """Gradient values a step must find zero: all of them, or with the binned scatter only those
        before the partitioned tables (the accumulate stores the rest; overflowed records go through
        the workspace's own words)."""
        if self._binned():
            return self.off_table + load().mfnerf_grid_binned_first_value(self.desc)
        return self.n_alloc

    def _grid_finish(self, q):
        """Fold part q's private copies of the coarse levels / convert the fixed-point sums."""
        call("mfnerf_grid_encode_bw_finish", self.desc, ptr(self.grads[self.off_table:]), ptr(self.parts[q].grid_ws),
             ptr(self._level_l1) if self._fixed() else None, stream())
        if self._fixed():
            self._level_l1.zero_()  # field_bw accumulates it; zeroed once used (also by adam_step_fixed)

    def _reduce_parts(self):
        """Fold parts 1.. MLP weight grads into grads (the table part is already shared)."""
        for t in self.parts[1:]:
            self.grads[:self.off_table].add_(t.mlp_grad)

    def _adam(self, grads, lo, hi, zero_grads):
        """Adam over params[lo:hi] with grads (hi-lo), refreshing p16[lo:hi]; a no-op (but for the
        zeroing) when the step's non-finite flag is up (raised by field_bw, cleared by the call)."""
        hyper, dev = self._adam_args()
        call("mfnerf_adam_step", ptr(self.params[lo:hi]), ptr(grads), ptr(self.m), ptr(self.v), ptr(self.p16[lo:hi]),
             hi - lo, *hyper, 1.0, 0, *dev, int(zero_grads), stream())

    def _finish_update(self, partial=False):
        """One part, unsharded, no exchange, after the scatter.  Fixed-point table gradient: the finish
        (convert) and Adam in one pass (mfnerf_adam_step_fixed), then the MLP weight repack; float
        atomics: the finish, then the plain update.  partial: after a fused _grid_bw, only the values
        before the partitioned tables (all of them if a slot overflowed)."""
        if not self._fixed():
            self._grid_finish(0)
            self._update()
            return
        ws, (hyper, dev) = self.parts[0].grid_ws, self._adam_args()
        args = (ptr(self.params), ptr(self.grads), ptr(self.m), ptr(self.v), ptr(self.p16), self.n_alloc,
                self.off_table, self.desc, ptr(ws), ptr(self._level_l1), *hyper, *dev)
        if partial:
            ovf = ctypes.c_void_p(ws.data_ptr() + load().mfnerf_grid_encode_bw_binned_flag_offset(
                self.desc, self._bin_slots()))
            call("mfnerf_adam_step_fixed_partial", *args,
                 self.off_table + load().mfnerf_grid_binned_first_value(self.desc), ovf, stream())
        else:
            call("mfnerf_adam_step_fixed", *args, stream())
        self._pack()

    def _update(self):
        """Adam over the flat params (+ fp16 mirror, + zeroing the gradient for the next step) +
        MLP weight repack (unsharded)."""
        self._adam(self.grads, 0, self.n_alloc, True)
        self._pack()

    def full_params(self):
        """The fp32 master parameters (all-gathered over ranks when the optimizer is sharded)."""
        if self.shard is None:
            return self.params
        from . import dp
        full = self.params.clone()
        dp.all_gather_(full, self.shard[0])
        return full

    def overflow_records(self):
        """Records the partitioned scatter could not place in their slots so far (added by integer
        atomics instead; a running total kept by the kernel; host read).  0 without partitions."""
        if not self._binned():
            return 0
        off = load().mfnerf_grid_encode_bw_binned_flag_offset(self.desc, self._bin_slots())
        ws = self.parts[0].grid_ws
        return int(ws.view(torch.int32)[off // 4 + 1])

    def skipped_steps(self):
        """Optimizer steps skipped on non-finite gradients so far (host read)."""
        return int(self.finite_status[1])

    def _count_update(self):
        """adam_step, the host's mirror of Adam's device-side step count: one more update issued."""
        self.adam_step += 1

    def _optimize(self, exchange, graphs=None):
        """The update half of a step.  Sharded: reduce-scatter -> Adam on the shard -> all-gather
        fp16 -> repack; else: exchange(grads) (all-reduce, optional) -> Adam -> repack.  graphs (a
        replay's): Adam and the repack are replays of the captured "adam" + "pack" / "update"."""
        from . import dp
        self._count_update()
        flag = self.finite_status[:1] if self._amp_on() else None
        if self.shard is not None:
            rank, lo, hi = self.shard

            def adam(g_shard):  # the flag holds the union over ranks by now (it rode the reduce-scatter)
                graphs["adam"].replay() if graphs else self._adam(g_shard, lo, hi, False)
            dp.sharded_update(self.grads, self.g_shard, self.p16, rank, adam, flag=flag)
            graphs["pack"].replay() if graphs else self._pack()
            return
        if exchange is not None:
            # the non-finite flag rides the all-reduce: NaN in element 0 when set, read back
            if flag is not None:
                call("mfnerf_flag_to_shards", ptr(self.grads), 1, self.n_alloc, ptr(flag), stream())
            exchange(self.grads)
            if flag is not None:
                call("mfnerf_flag_from_shard", ptr(self.grads), ptr(flag), stream())
        graphs["update"].replay() if graphs else self._update()

    def _check_bg(self, *given):
        """bg= / next_bg= are for a step that passes its batches with random_bg on (ignored on a
        synthetic scene, like the flag): an attached dataset's draw writes the colour itself."""
        if all(b is None for b in given):
            return
        if not self.cfg.random_bg:
            raise ValueError("bg= needs StepConfig(random_bg=True)")
        if self.dataset is not None:
            raise ValueError("bg= is for batches the caller passes: the attached dataset's draw writes the colour")

    def run(self, batch: Batch = None, mark=None, exchange=None, optimize=True, noise=None, bg=None):
        """One training step, eagerly on the current stream, parts in sequence, march buffer set 0.
        mark(name) is called after each stage (bench timing); exchange(grads) runs between backward
        and Adam (the data-parallel all-reduce).  batch=None: drawn from the attached dataset.
        optimize=False stops after the backward and leaves the step's gradient in self.grads (no
        Adam step, no repack; for inspection).  random_bg: the step's background colour comes with
        the dataset's draw; for a passed batch it is bg (3 values) or, bg=None, three draws from the
        step's generator after the noise."""
        mark = mark or _nomark
        self._check_bg(bg)
        self._check_hdr(exchange)
        if self.cfg.refine_poses:
            self._check_refine(exchange)
            if batch is not None:
                raise ValueError("refine_poses draws its batch from the attached dataset: pass no batch")
        self._flush_pack()
        mb = self.mbuf[0]
        prepped = batch is None
        if prepped:
            batch = self._sampled
            self._draw(batch, mb)
        elif self.cfg.hdr:
            self._stage_exposure(batch, mb)
        self._use(mb)
        self.last_batch = batch
        self._primed = False  # a pipelined replay() must march its own batch next
        self._march(batch, mb, mark, prepped=prepped, noise=noise, bg=bg)
        if self.n_parts == 1 and self._dp(exchange):
            self._dp_backward(batch, mb, mark)
        else:
            for q in range(self.n_parts):
                self._chain(batch, mb, q, mark, side_adam=optimize)
                self._grid_bw(mb, q)
                mark("grid_bw")
                self._grid_finish(q)
                mark("grid_finish")
        self._reduce_parts()
        if optimize:
            self._optimize(exchange)
        mark("update")

    def set_lr(self, lr):
        """Device-resident learning rate (train.py:137-142 cosine schedule), read by Adam."""
        self.lr_dev.fill_(float(lr))

    def step(self, batch: Batch):
        self.run(batch)

    # ------------------------------- the step's forms: one body each, launched by run(), recorded by capture()
    def _dp(self, exchange):
        """Data parallel: a sharded optimizer, or a gradient exchange between backward and Adam."""
        return self.shard is not None or exchange is not None

    def _fused_shard(self):
        """Sharded with amp: one launch reads the exchanged flag, updates and zeroes level_l1."""
        return self._amp_on() and self.shard is not None

    def _dp_backward(self, batch, mb, mark=_nomark, captured=False):
        """Data parallel, one part: the chain, then the table gradient scattered and finished to floats
        for the exchange (binned: the accumulate writes the partitioned tables' floats and one finish
        pass covers the rest).  Eagerly _flush_pack precedes and _optimize follows, carrying the
        non-finite flag around its own collective.  The captured form (dp_pre) differs in four ways:
        it starts with the repack; it opens the gate; the flag rides the collective as NaN in every
        shard's first value (written by the float finish when it has a table prefix to ride, else by a
        launch of its own); level_l1 is left to the sharded Adam, whose last workgroup zeroes it."""
        gate, flag_rides = None, False
        if captured:
            self._pack()  # the previous step's all-gathered / updated fp16 weights
            gate, flag_rides = self._gate_ptr(), self._amp_on()
            w = self.shard[2] - self.shard[1] if self.shard is not None else self.n_alloc
            flag, shards = ptr(self.finite_status), (self.n_alloc // w, w)  # (how many, how long)
        self._chain(batch, mb, 0, mark)
        if self._binned():
            src, table, binned_ws = self._scatter_args(mb, 0)
            self._open_gate(gate, in_launch=True)
            fold = flag_rides and load().mfnerf_grid_binned_first_value(self.desc) > 0
            call("mfnerf_grid_encode_bw_binned_float", *src, table, *binned_ws, gate,
                 *((flag, *shards) if fold else (None, 0, 0)), self.off_table, stream())
            if not (captured and self._fused_shard()):
                self._level_l1.zero_()
            flag_rides = flag_rides and not fold
        else:
            self._grid_bw(mb, 0, gate=gate)
            self._grid_finish(0)
        if flag_rides:
            call("mfnerf_flag_to_shards", ptr(self.grads), *shards, flag, stream())
        mark("grid_bw")
        mark("grid_finish")

    def _dp_post(self):
        """After the exchange: the flag back, then Adam on this rank's shard (sharded) or everywhere."""
        g, lo, hi = (self.g_shard, *self.shard[1:]) if self.shard is not None else (self.grads, 0, self.n_alloc)
        if self._fused_shard():
            # mfnerf_adam_step_shard: the flag_from_shard launch and the level_l1 fill folded in
            hyper, dev = self._adam_args()
            call("mfnerf_adam_step_shard", ptr(self.params[lo:hi]), ptr(g), ptr(self.m), ptr(self.v),
                 ptr(self.p16[lo:hi]), hi - lo, *hyper, 1.0, *dev, ptr(self._level_l1), self._level_l1.numel(),
                 stream())
            return
        if self._amp_on():
            call("mfnerf_flag_from_shard", ptr(g), ptr(self.finite_status), stream())
        self._adam(g, lo, hi, self.shard is None)

    def _dp_exchange(self, exchange, update):
        """The collectives around the data-parallel update (update: _dp_post, or its graph's replay)."""
        from . import dp
        if self.shard is None:
            exchange(self.grads)
            return update()
        dp.reduce_scatter_mean_(self.g_shard, self.grads)
        update()
        dp.all_gather_(self.p16, self.shard[0])

    def _dp_step(self, j):
        """RCCL on this stream (mfnerf.rccl): the collectives are captured too, and the whole
        data-parallel step (repack, chain, scatter, exchange, Adam, all-gather) replays as ONE graph
        -- no host hop between the backward and the update."""
        from . import dp
        self._dp_backward(self._static[j], self.mbuf[j], captured=True)
        self._dp_exchange(dp.allreduce_mean_, self._dp_post)

    def _march_static(self, j, gated=False):
        """Static set j (the dataset's draw, or what replay() staged) into march buffer set j."""
        if gated:
            call("mfnerf_gate_wait", self._gate_ptr(), GATE_TIMEOUT_US, stream())
        drawn = self.dataset is not None
        if drawn:
            self._draw(self._static[j], self.mbuf[j])
        self._march(self._static[j], self.mbuf[j], _nomark, prepped=drawn,
                    noise=self._static_noise[j] if self._host_noise else None,
                    bg=self._static_bg[j] if self._static_bg is not None else None)

    def _step(self, j, whole=True):
        """The collective-free step on set j.  whole: from the chain, as ONE graph whose scatter opens
        the device gate where the host used to record the event that starts the next march; else from
        the scatter on (per-stage steps).  Where the layout allows, the whole optimizer runs inside the
        scatter's launches (the MLPs' and dense levels' update rides the accumulate's, then the repack)."""
        gate = self._gate_ptr() if whole else None
        if whole:
            self._chain(self._static[j], self.mbuf[j], 0, _nomark)
        if self._fused_adam_ok():
            self._grid_bw(self.mbuf[j], 0, fuse_adam="all", gate=gate)
        else:
            self._grid_bw(self.mbuf[j], 0, gate=gate)
            self._finish_update()

    # ---------------------------------------------------------------- HIP graphs
    def capture(self, host_noise=False):
        """Capture the step as HIP graphs over two alternating march buffer sets j = 0, 1.

        One part, no collective (the default N=1 step): ONE graph per step ("step": chain -> scatter
        with the whole optimizer in its launches -> repack); the next step's batch draw + march is a
        graph of its own on a side stream, started by a device gate the step graph opens as the
        table-gradient scatter begins (gate.hip).  Data parallel (one part): TWO graphs per step around
        the collective ("dp_pre": repack -> chain -> scatter -> float gradient -> non-finite flag
        into the shards; "dp_post": flag back -> Adam on this rank's shard (sharded) or everywhere
        (all-reduce)), the collectives issued stream-ordered between them, the march gated the same
        way.  The per-stage graphs (march[j], chain[j][q], grid_bw[j][q], finish, update / adam +
        pack) serve several parts and the steps whose scatter is timed by events (bench).
        host_noise: the march perturbation is copied from a buffer replay(noise=...) fills instead of
        drawn from the step's generator (parity tests driving several processes with one draw); with
        random_bg and no attached dataset the background colour is staged the same way
        (replay(bg=, next_bg=)).  random_bg: the colour is part of the march graph (the dataset's draw
        launch, or the generator / staged copy), written into the march buffer set the batch goes
        into, so the step graph of set j reads the colour of the batch it trains on while the next
        batch's colour waits in set 1-j.
        Call after at least one eager step (lazy library init happens outside capture)."""
        self._check_refine()
        self._check_hdr()
        self._flush_pack()
        self._capture_setup(host_noise)
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()

        def cap(fn, *args, rng=False, **kw):
            g = torch.cuda.CUDAGraph()
            if rng:
                g.register_generator_state(self.gen)
            with torch.cuda.graph(g, pool=pool):
                fn(*args, **kw)
            return g

        # (the order of the captures is kept as it was: they share one memory pool)
        self.graphs = self._capture_stages(cap)
        if self.n_parts == 1:
            self.graphs.update(self._capture_dp(cap))
            if self.shard is None:
                self.graphs.update(self._capture_one_graph(cap))
        n_gated = 2 * sum(1 for k in ("step", "dp_pre", "dp_step") if self.graphs.get(k) is not None)
        if self._gate is not None and self._gate_opened != n_gated:
            # every gated graph must open the gate exactly once, or each gated march would spin for
            # GATE_TIMEOUT_US before starting
            raise RuntimeError(f"gated graphs opened the gate {self._gate_opened} times, not {n_gated}")
        torch.cuda.synchronize()

    def _capture_setup(self, host_noise):
        """What replay() fills (second march buffer set, static batches, host_noise's staged noise / colour)
        and orders the graphs with (the gated march's gate, streams, events); set 0 first, unprimed."""
        N, dev, P = self.cfg.n_rays, self.dev, self.n_parts
        if len(self.mbuf) == 1:
            self.mbuf.append(self._march_buffers())
        if self.cfg.refine_poses:
            self.compose_poses()  # both buffers start from the offsets the eager steps left
        self._static = [_packed_batch(torch.zeros(3, N, 3, device=dev)) for _ in range(2)]
        self._host_noise = bool(host_noise)
        self._static_noise = [torch.zeros(N, device=dev) for _ in range(2)] if host_noise else None
        host_bg = host_noise and self._random_bg() and self.dataset is None
        self._static_bg = [torch.zeros(3, device=dev) for _ in range(2)] if host_bg else None
        # one part: the next step's march waits on the side stream for the gate the step graph opens
        # as its scatter begins (the dense-level launch's first workgroup, or a signal kernel)
        self._gate = torch.zeros(4, dtype=torch.int32, device=dev) if P == 1 else None
        self._gate_opened = 0
        # the side stream at normal queue priority: a high-priority one measured the same alone
        # (0.601 vs 0.601 ms/step) but, once an RCCL communicator exists in the process, it ran every
        # step at 1.10 ms (kernels on the main queue 2-7x slower; the extra streams share hardware
        # queues) -- the data-parallel step would pay it on every rank.  No priority below normal
        # exists here (torch.cuda.Stream.priority_range() is (0, -1) on this ROCm, r4m).
        self._side = torch.cuda.Stream(device=dev, priority=0)
        self._part_streams = [None] + [torch.cuda.Stream(device=dev) for _ in range(P - 1)]
        self._ev_march = [torch.cuda.Event(), torch.cuda.Event()]
        self._ev_start = torch.cuda.Event()
        self._ev_chain = [torch.cuda.Event() for _ in range(P)]
        self._ev_part = [torch.cuda.Event() for _ in range(P)]
        self._parity = 0
        self._primed = False

    def _gate_ptr(self):
        return ptr(self._gate) if self._gate is not None else None

    def _capture_stages(self, cap):
        """The per-stage graphs: march (and, one part, gated march), chain, scatter, finish, reduce, update."""
        P, sets = self.n_parts, range(2)
        g = {
            "march": [cap(self._march_static, j, rng=True) for j in sets],
            "chain": [[cap(self._chain, self._static[j], self.mbuf[j], q, _nomark) for q in range(P)] for j in sets],
            "grid_bw": [[cap(self._grid_bw, self.mbuf[j], q) for q in range(P)] for j in sets],
            "finish": [cap(self._grid_finish, q) for q in range(P)],
            "reduce": cap(self._reduce_parts) if P > 1 else None,
        }
        if self._gate is not None:
            g["march_gated"] = [cap(self._march_static, j, gated=True, rng=True) for j in sets]
        g["pack"] = cap(self._pack)
        if self.shard is not None:
            g["adam"] = cap(self._adam, self.g_shard, self.shard[1], self.shard[2], False)
        else:
            g["update"] = cap(self._update)
        return g

    def _capture_dp(self, cap):
        """One part, data parallel: up to the exchange, after it and, direct RCCL, both around it as one graph."""
        from . import dp
        g = {"dp_pre": [cap(self._dp_backward, self._static[j], self.mbuf[j], captured=True) for j in range(2)],
             "dp_post": cap(self._dp_post)}
        if dp.direct_rccl() is not None:
            g["dp_step"] = [cap(self._dp_step, j) for j in range(2)]
        return g

    def _capture_one_graph(self, cap):
        """One part, no collective: the tail, the scatter with it (untimed per-stage steps), the whole step."""
        return {"finish_update": cap(self._finish_update),
                "grid_bw_tail": [cap(self._step, j, whole=False) for j in range(2)],
                "step": [cap(self._step, j) for j in range(2)]}

    def gate_timeouts(self):
        """Gated marches that started on the gate's timeout instead of its signal (gate.hip's gate[3],
        cumulative; a host read, so it synchronises): non-zero means a step paid up to GATE_TIMEOUT_US
        -- e.g. the side stream shares a hardware queue with the stream that signals."""
        return 0 if self._gate is None else int(self._gate[3])

    def _march_on_side(self, j, batch, after, gated=False, noise=None, bg=None):
        """Copy batch (and, captured with host_noise, its perturbation and, random_bg without a dataset,
        its background colour) into static set j and march it on the side stream once `after` (an
        event on the main stream) has passed: set j's buffers were last read two steps back.  gated:
        the march graph first waits (a polling wave, at most GATE_TIMEOUT_US) for the step graph's
        gate signal (placement only)."""
        self._side.wait_event(after)
        with torch.cuda.stream(self._side):
            dst = self._static[j]
            if batch is not None and batch.buf is not None:
                dst.buf.copy_(batch.buf)
            elif batch is not None:
                for d, s_ in zip((dst.rays_o, dst.rays_d, dst.rgb), (batch.rays_o, batch.rays_d, batch.rgb)):
                    d.copy_(s_)
            if self.cfg.hdr and batch is not None:
                self._stage_exposure(batch, self.mbuf[j])
            if self._host_noise:
                if noise is None:
                    raise ValueError("captured with host_noise: pass noise= / next_noise= to replay()")
                self._static_noise[j].copy_(noise)
            if self._static_bg is not None:
                if bg is None:
                    raise ValueError("captured with host_noise and random_bg: pass bg= / next_bg= to replay()")
                self._static_bg[j].copy_(torch.as_tensor(bg, dtype=torch.float32).reshape(3))
            self.graphs["march_gated" if gated else "march"][j].replay()
            self._ev_march[j].record(self._side)

    def replay(self, batch: Batch = None, exchange=None, grid_bw_events=None, next_batch=None, prefetch=None,
               noise=None, next_noise=None, bg=None, next_bg=None):
        """One training step from the captured graphs (the kernels of run()).  With next_batch (or,
        with an attached dataset, prefetch=True, its default), the next step's march is issued on
        the side stream to overlap this step; the next replay() must then be called with that batch
        (or, with a dataset, the next replay() trains on the batch already drawn).  Pass
        prefetch=False before anything that must precede the next march (an occupancy refresh).
        Data parallel: sharded (shard_optimizer) or exchange=dp.allreduce_mean_.
        grid_bw_events: optional (start, [end per part]) timing events -- start before part 0's
        grid_bw, end after each part's grid_bw (that step runs the per-stage graphs).
        noise / next_noise: the perturbations of batch / next_batch (capture(host_noise=True));
        bg / next_bg: their background colours (random_bg, capture(host_noise=True), no dataset)."""
        j = self._parity
        self._check_refine(exchange)
        self._check_hdr(exchange)
        self._check_bg(bg, next_bg)
        if self.dataset is not None:
            batch = None
            if prefetch is None:
                prefetch = True
        elif prefetch is None:
            prefetch = next_batch is not None
        elif prefetch and next_batch is None:
            raise ValueError("prefetch needs next_batch (or an attached dataset)")
        main = torch.cuda.current_stream()
        self._ev_start.record(main)
        if not self._primed:
            self._march_on_side(j, batch, self._ev_start, noise=noise, bg=bg)
        self._use(self.mbuf[j])
        self.last_batch = self._static[j]
        nxt = dict(batch=next_batch, noise=next_noise, bg=next_bg)
        # one part, prefetching, no scatter to time: the step is one graph (two around a host-issued
        # collective) and the next march starts at its gate signal; else the per-stage graphs
        if self._gate is not None and grid_bw_events is None and prefetch:
            self._replay_one_graph(j, main, exchange, nxt)
        else:
            self._replay_stages(j, main, exchange, grid_bw_events, nxt if prefetch else None)
        self._parity = 1 - j
        self._primed = bool(prefetch)

    def _replay_one_graph(self, j, main, exchange, nxt):
        """Set j's step as one graph -- "step", or data parallel "dp_step" (direct RCCL: collectives
        included) or "dp_pre" -> collective -> "dp_post" -> (all-gather) -- with set 1-j's gated march
        issued behind it on the side stream."""
        from . import dp
        g, dp_mode = self.graphs, self._dp(exchange)
        # set 1-j was last read by the previous step, all of which precedes _ev_start
        main.wait_event(self._ev_march[j])
        self._count_update()
        key = "dp_pre" if dp_mode else "step"
        if dp_mode and g.get("dp_step") is not None and (self.shard is not None or exchange is dp.allreduce_mean_):
            key = "dp_step"  # direct RCCL: the collectives are in the graph
        g[key][j].replay()
        self._march_on_side(1 - j, after=self._ev_start, gated=True, **nxt)
        if key == "dp_pre":
            self._dp_exchange(exchange, g["dp_post"].replay)
        self._stale_pack = dp_mode  # the next step's dp_pre / dp_step graph (or _flush_pack) repacks

    def _replay_stages(self, j, main, exchange, grid_bw_events, nxt):
        """Set j's step from the per-stage graphs, part q > 0 on its own stream; nxt: set 1-j's march or None."""
        g, P, timed = self.graphs, self.n_parts, grid_bw_events is not None
        fuse_tail = P == 1 and not self._dp(exchange)  # the collective-free tail graphs exist and apply
        self._flush_pack()
        main.wait_event(self._ev_march[j])
        for q in range(P):
            sq = main if q == 0 else self._part_streams[q]
            if q > 0:
                sq.wait_event(self._ev_chain[q - 1])
            with torch.cuda.stream(sq):
                g["chain"][j][q].replay()
                self._ev_chain[q].record(sq)
                if q == P - 1 and nxt is not None:
                    # set 1-j was last read by the previous step, which this chain follows; waiting
                    # for the last chain puts the march under the grid_bw scatters, not the chains
                    self._march_on_side(1 - j, after=self._ev_chain[q], **nxt)
                if fuse_tail and not timed:
                    # P == 1: scatter + convert/Adam + repack as one graph (no event needed between)
                    self._count_update()
                    g["grid_bw_tail"][j].replay()
                else:
                    if timed and q == 0:
                        grid_bw_events[0].record(sq)
                    g["grid_bw"][j][q].replay()
                    if timed:
                        grid_bw_events[1][q].record(sq)
                    if q > 0:  # the folds read-modify-write the shared gradient: one part at a time
                        sq.wait_event(self._ev_part[q - 1])
                    if not fuse_tail:
                        g["finish"][q].replay()
                self._ev_part[q].record(sq)
        for q in range(1, P):
            main.wait_event(self._ev_part[q])
        if g["reduce"] is not None:
            g["reduce"].replay()
        if not fuse_tail:
            self._optimize(exchange, graphs=g)
        elif timed:  # (untimed: replayed with the scatter above)
            self._count_update()
            g["finish_update"].replay()

    # ---------------------------------------------------------------- occupancy (networks.py:157-271)
    def _occ_buffers(self):
        """Scratch for the refresh, sized for the warm-up (all cells) case, allocated once."""
        if self._occ is None:
            lib, c, C, G = load(), self.cfg, self.cascades, self.G
            # one point per distinct drawn cell (mfnerf_occupancy_cells_unique_dev): at most every cell
            n = max(lib.mfnerf_occupancy_points_unique(C, G, G ** 3 // 4, 0), lib.mfnerf_occupancy_points(C, G, 0, 1))
            o = _State()
            o.n_max = n
            o.xyz = torch.empty(n, 3, dtype=torch.float32, device=self.dev)
            o.cell = torch.empty(n, dtype=torch.int32, device=self.dev)
            o.feat = torch.empty(c.L, n, c.F, dtype=torch.float16, device=self.dev)  # level planes
            o.sigma = torch.empty(n, dtype=torch.float32, device=self.dev)
            o.tmp = torch.zeros(C * G ** 3, dtype=torch.float32, device=self.dev)  # kept zero by the decay
            o.ws = torch.zeros(lib.mfnerf_occupancy_workspace(C, G), dtype=torch.uint8, device=self.dev)
            o.count = torch.zeros(1, dtype=torch.int32, device=self.dev)  # probed (distinct) cells
            o.calls = torch.zeros(1, dtype=torch.int64, device=self.dev)  # the draws' call index (device)
            o.graphs = {}
            self._occ = o
        return self._occ

    @torch.no_grad()
    def update_density_grid(self, warmup=False, decay=0.95, count_grid=None, seed=0):
        """NGP.update_density_grid(0.01*MAX_SAMPLES/sqrt(3), warmup, erode) as device launches only
        (cells -> grid_encode_fw -> field_fw density-only + scatter -> decay/mean -> thr + packbits); no
        host synchronisation.  Without erosion (count_grid) the launches are captured once per
        (warmup, decay, seed) and replayed as one HIP graph (the draws' call index lives on the
        device, so every replay draws new cells): 0.45 ms of mostly launch overhead eagerly
        (DESIGN.md 6)."""
        o = self._occ_buffers()
        self._flush_pack()  # the density query runs the field on `packed`
        if count_grid is not None:
            self._occ_launches(warmup, decay, count_grid, seed)
            return
        key = (bool(warmup), float(decay), int(seed))
        g = o.graphs.get(key)
        if g is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._occ_launches(warmup, decay, None, seed)
            o.graphs[key] = g  # (capturing ran nothing)
        g.replay()

    def _occ_launches(self, warmup, decay, count_grid, seed):
        c, C, G, s = self.cfg, self.cascades, self.G, stream()
        o = self._occ_buffers()
        M = G ** 3 // 4
        # the draws of sample_uniform_and_occupied_cells / get_all_cells reduced to one jittered point per
        # distinct drawn cell (the only sigmas the grid can keep), in row-major cell order; count on the device
        n = load().mfnerf_occupancy_points_unique(C, G, M, int(warmup))
        call("mfnerf_occupancy_cells_unique_dev", ptr(self.density_grid), C, G, float(c.scale), M, int(warmup),
             DENSITY_THRESHOLD, seed, ptr(o.calls), ptr(o.xyz), ptr(o.cell), ptr(o.count), ptr(o.ws), s)
        call("mfnerf_grid_encode_fw_planar", ptr(o.xyz), n, ptr(o.count), self.x_min, self.x_range, self.desc,
             ptr(self.p16[self.off_table:]), ptr(o.feat), o.n_max, s)
        # sigma + density_grid_tmp[cell] = sigma in one launch; the update then starts at the decay
        call("mfnerf_field_fw_density_scatter", ptr(o.feat), o.n_max, n, ptr(o.count), ptr(self.packed), c.rgb_width,
             ptr(o.sigma), ptr(o.cell), ptr(o.tmp), s)
        call("mfnerf_occupancy_update_dev", ptr(self.density_grid), None, None, 0, None, C, G, float(decay),
             ptr(count_grid) if count_grid is not None else None, DENSITY_THRESHOLD, ptr(o.tmp), 1,
             ptr(self.bitfield), ptr(o.ws), s)
