/*
 * mfnerf.h -- C ABI of libmfnerf_hip.so, the MI355X (gfx950) kernels behind MF-NeRF's
 * volumetric-rendering training step.
 *
 * Conventions (every entry point):
 *   - plain device pointers + sizes, row-major contiguous arrays, no torch types;
 *   - the last argument is the HIP stream the work is enqueued on (NULL = legacy default);
 *   - return 0 on success, a nonzero MFN_ERR_* code otherwise; mfnerf_last_error()
 *     returns a message for the calling thread's last failure;
 *   - no entry point allocates, frees or synchronises: callers pass workspace, so every
 *     call is legal inside hipStreamBeginCapture (HIP graphs);
 *   - outputs are NOT pre-zeroed by the library unless stated ("zero-fills").
 *
 * Reference interfaces replaced (lly00412/MF-NeRF, paths relative to the repo root):
 *   vren pybind module: models/csrc/binding.cpp:234-250 (C++ signatures binding.cpp:4-231,
 *   models/csrc/include/utils.h:9-126); tiny-cuda-nn HashGrid / SphericalHarmonics /
 *   FullyFusedMLP as configured in models/networks.py:36-79; apex FusedAdam (train.py:136);
 *   torchmetrics PSNR / SSIM of the validation step (train.py:65-67, 198-237).
 */
#ifndef MFNERF_H
#define MFNERF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mfnerf_stream_t; /* == hipStream_t */

#define MFN_OK 0
#define MFN_ERR_INVALID 1 /* bad argument (null pointer, bad size, unsupported config) */
#define MFN_ERR_LAUNCH 2  /* HIP launch error */

const char* mfnerf_last_error(void);
int mfnerf_abi_version(void);

/* Mixed-precision state of a training step, device-resident (32 bytes, zero-initialised by the
 * caller, then scale / growth_interval / growth_factor / backoff_factor set): torch.cuda.amp.GradScaler
 * as PyTorch-Lightning's precision=16 drives it (train.py:287; init scale 65536, growth 2.0 every
 * 2000 clean steps, backoff 0.5).  Producers of the step's gradient raise `nonfinite`; the optimizer
 * call skips the update when it is set and then runs GradScaler.update() on the device.
 * growth_interval == 0: static scaling (the skip only; mfnerf_field_bw then uses its grad_scale). */
typedef struct {
    int32_t nonfinite;       /* 1 when some gradient of the step is inf/nan; cleared by the optimizer */
    int32_t skipped;         /* optimizer steps skipped so far */
    float scale;             /* current loss scale (dynamic mode) */
    int32_t growth_tracker;  /* clean steps since the last scale change */
    int32_t growth_interval; /* 2000; 0 = static */
    float growth_factor;     /* 2.0 */
    float backoff_factor;    /* 0.5 */
    int32_t ticket;          /* the optimizer pass's last-workgroup ticket; 0 between calls */
} mfnerf_amp_state;

/* ---------------------------------------------------------------- vren ops */

/* vren.ray_aabb_intersect (binding.cpp:4-16, intersection.cu:59-100).
 * rays_o, rays_d (n_rays,3) f32; centers, half_sizes (n_voxels,3) f32.
 * Writes hit_cnt (n_rays) i32, hits_t (n_rays,max_hits,2) f32, hits_voxel_idx (n_rays,max_hits) i64;
 * zero-fills / -1-fills all three.  Hits are kept in voxel order and sorted near->far by t1. */
int mfnerf_ray_aabb_intersect(const float* rays_o, const float* rays_d, const float* centers,
                              const float* half_sizes, int64_t n_rays, int64_t n_voxels, int max_hits,
                              int32_t* hit_cnt, float* hits_t, int64_t* hits_voxel_idx, mfnerf_stream_t stream);

/* vren.morton3D (binding.cpp:46-50, raymarching.cu:62-88): coords (n,3) i32 -> out (n) i32. */
int mfnerf_morton3d(const int32_t* coords, int64_t n, int32_t* out, mfnerf_stream_t stream);

/* vren.morton3D_invert (binding.cpp:53-57, raymarching.cu:90-119): idx (n) i32 -> coords (n,3) i32. */
int mfnerf_morton3d_invert(const int32_t* idx, int64_t n, int32_t* coords, mfnerf_stream_t stream);

/* vren.packbits (binding.cpp:34-43, raymarching.cu:122-161): bit i of byte n = grid[8n+i] > thr.
 * grid (8*n_bytes) f32.  thr_dev, when non-NULL, is a device f32 read instead of `thr`
 * (keeps the occupancy update free of host syncs). */
int mfnerf_packbits(const float* grid, int64_t n_bytes, float thr, const float* thr_dev, uint8_t* bitfield,
                    mfnerf_stream_t stream);

/* Workspace bytes mfnerf_raymarching_train needs for n_rays rays of at most max_samples samples
 * (the per-ray counts, and the march's per-ray sample positions t: n_rays x max_samples f32). */
int64_t mfnerf_raymarching_train_workspace(int64_t n_rays, int max_samples);

/* vren.raymarching_train (binding.cpp:60-85, raymarching.cu:166-332).
 * hits_t: (n_rays,2) f32 rows (t1,t2) with row stride hits_stride floats.
 * Outputs: rays_a (n_rays,3) i64 -- row r = (r, start, count), start = exclusive prefix sum
 *          (canonical order; the reference's atomicAdd order is nondeterministic);
 *          xyzs, dirs (capacity,3), deltas, ts (capacity) f32 -- samples [0, counter[0]);
 *          counter (2) i32 = (total samples, n_rays).  Samples beyond `capacity` are dropped
 *          (their rays' counts are clipped).  Device-resident count: no host sync. */
int mfnerf_raymarching_train(const float* rays_o, const float* rays_d, const float* hits_t, int64_t hits_stride,
                             const uint8_t* bitfield, int cascades, float scale, float exp_step_factor,
                             const float* noise, int grid_size, int max_samples, int64_t n_rays, int64_t capacity,
                             int64_t* rays_a, float* xyzs, float* dirs, float* deltas, float* ts, int32_t* counter,
                             void* workspace, mfnerf_stream_t stream);

/* vren.raymarching_test (binding.cpp:88-115, raymarching.cu:335-454), including the reference's
 * calc_dt(..., cascades) quirk.  hits_t (n_rays,2 with row stride hits_stride) is updated in place
 * (column 0).  Zero-fills xyzs, dirs (n_alive,N_samples,3), deltas, ts (n_alive,N_samples), n_eff (n_alive) i32. */
int mfnerf_raymarching_test(const float* rays_o, const float* rays_d, float* hits_t, int64_t hits_stride,
                            const int64_t* alive_indices, int64_t n_alive, const uint8_t* bitfield, int cascades,
                            float scale, float exp_step_factor, int grid_size, int max_samples, int N_samples,
                            float* xyzs, float* dirs, float* deltas, float* ts, int32_t* n_eff,
                            mfnerf_stream_t stream);

/* vren.composite_train_fw (binding.cpp:118-136, volumerendering.cu:6-84).
 * sigmas (n_samples), rgbs (n_samples,3), deltas, ts f32; rays_a (n_rays,3) i64.
 * Writes total_samples (indexed by ray id) i64, opacity, depth (n_rays), rgb (n_rays,3) and ws for every
 * sample of every listed ray (0 after the ray terminates); no memset of n_samples-sized buffers. */
int mfnerf_composite_train_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                              const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                              int64_t* total_samples, float* opacity, float* depth, float* rgb, float* ws,
                              mfnerf_stream_t stream);

/* vren.composite_train_bw (binding.cpp:139-173, volumerendering.cu:87-202).  Writes dL_dsigmas (n_samples)
 * and dL_drgbs (n_samples,3) for every sample of every listed ray (0 after the ray terminates).
 * The per-ray scan of dL_dws*ws (host-side + thrust in the reference) is done in-kernel. */
int mfnerf_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                              const float* dL_dws, const float* sigmas, const float* rgbs, const float* ws,
                              const float* deltas, const float* ts, const int64_t* rays_a, const float* opacity,
                              const float* depth, const float* rgb, int64_t n_rays, int64_t n_samples,
                              float T_threshold, float* dL_dsigmas, float* dL_drgbs, mfnerf_stream_t stream);

/* Fused training compositing for the default loss (no distortion term): mfnerf_composite_train_fw,
 * mfnerf_nerf_loss (target, n_mean, lambda_opacity, bg) and mfnerf_composite_train_bw with
 * dL_ddepth = 0, dL_dws = 0 in one pass (one wave per ray); the same outputs as the three calls,
 * bit-identical.  loss_partials (optional, ceil(n_rays/4) device f32) is OVERWRITTEN with the loss
 * value as one partial sum per 4 rays (their sum is the loss; no zeroing needed).  Replaces the chain at rendering.py:121-163 + losses.py:47-60
 * + custom_functions.py:148-159 in one training step. */
int mfnerf_composite_train_fused(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                                 const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                                 const float* target, int64_t n_mean, float lambda_opacity, float bg_r, float bg_g,
                                 float bg_b, int64_t* total_samples, float* opacity, float* depth, float* rgb,
                                 float* ws, float* dL_drgb, float* dL_dopacity, float* dL_dsigmas, float* dL_drgbs,
                                 float* loss_partials, mfnerf_stream_t stream);

/* mfnerf_composite_train_fused with the background colour read from device memory: bg (3 f32,
 * device, required) in place of bg_r, bg_g, bg_b.  For --random_bg (rendering.py:153-161: one random
 * colour per training batch, blended into the prediction only), where the colour is drawn on the device
 * and a captured graph would freeze scalar arguments.  The same kernel, specialised at compile time;
 * the three values are read once per ray before the sample loop, the arithmetic and its order are
 * those of the scalar form: with equal values every output is bit-identical. */
int mfnerf_composite_train_fused_bg(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                                    const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                                    const float* target, int64_t n_mean, float lambda_opacity, const float* bg,
                                    int64_t* total_samples, float* opacity, float* depth, float* rgb, float* ws,
                                    float* dL_drgb, float* dL_dopacity, float* dL_dsigmas, float* dL_drgbs,
                                    float* loss_partials, mfnerf_stream_t stream);

/* vren.composite_test_fw (binding.cpp:176-201, volumerendering.cu:205-285).  sigmas (n_alive,N_samples),
 * rgbs (n_alive,N_samples,3), deltas, ts (n_alive,N_samples); in place on alive_indices, opacity,
 * depth, rgb (indexed by ray). */
int mfnerf_composite_test_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                             int64_t* alive_indices, int64_t n_alive, int N_samples, float T_threshold,
                             const int32_t* n_eff, float* opacity, float* depth, float* rgb,
                             mfnerf_stream_t stream);

/* vren.distortion_loss_fw (binding.cpp:204-216, losses.cu:9-109).  Zero-fills loss (n_rays) and
 * writes ws_inclusive_scan, wts_inclusive_scan (n_samples). */
int mfnerf_distortion_loss_fw(const float* ws, const float* deltas, const float* ts, const int64_t* rays_a,
                              int64_t n_rays, int64_t n_samples, float* loss, float* ws_incl, float* wts_incl,
                              mfnerf_stream_t stream);

/* vren.distortion_loss_bw (binding.cpp:219-231, losses.cu:112-175).  Zero-fills dL_dws (n_samples). */
int mfnerf_distortion_loss_bw(const float* dL_dloss, const float* ws_incl, const float* wts_incl,
                              const float* ws, const float* deltas, const float* ts, const int64_t* rays_a,
                              int64_t n_rays, int64_t n_samples, float* dL_dws, mfnerf_stream_t stream);

/* NeRFLoss (losses.py:47-60) + the background blend (rendering.py:153-161) and its gradient, fused:
 * pred = rgb + bg*(1-opacity); loss = mean((pred-target)^2) + lambda_opacity*mean(-o ln o),
 * o = opacity+1e-10 (train.py:178 sums the two means).  Writes dL_drgb (n,3), dL_dopacity (n);
 * loss_sum (optional, device f32) is ACCUMULATED with the loss value.  n_mean: the ray count the
 * means are taken over (0 = n_rays); a batch computed in parts passes the full batch size so the
 * parts' losses and gradients add up to the whole batch's. */
int mfnerf_nerf_loss(const float* rgb, const float* opacity, const float* target, int64_t n_rays, int64_t n_mean,
                     float lambda_opacity, float bg_r, float bg_g, float bg_b, float* dL_drgb, float* dL_dopacity,
                     float* loss_sum, mfnerf_stream_t stream);

/* mfnerf_nerf_loss with the background colour read from device memory (bg: 3 f32, device, required;
 * --random_bg, rendering.py:153-161), once per thread; the same kernel specialised at compile time,
 * bit-identical to the scalar form for equal values. */
int mfnerf_nerf_loss_bg(const float* rgb, const float* opacity, const float* target, int64_t n_rays, int64_t n_mean,
                        float lambda_opacity, const float* bg, float* dL_drgb, float* dL_dopacity, float* loss_sum,
                        mfnerf_stream_t stream);

/* ---------------------------------------------------------------- grid encoding (tcnn HashGrid / MF) */

/* Level table of a multiresolution grid (tcnn GridEncodingTemplated, networks.py:39-49).
 * Host-computed once; per level: scale = exp2f(l*log2f(b))*N_min - 1, res = ceil(scale)+1,
 * offset/size in entries (of n_features values each).  table_kind: 0 own table (dense when
 * res^3 <= size, else coherent prime hash), 1 MixedFeature shared table (canonical-grid index). */
#define MFN_MAX_LEVELS 32
typedef struct {
    int32_t n_levels;
    int32_t n_features;         /* F: only 2 is supported by the kernels */
    int32_t canon_res;          /* MixedFeature canonical grid resolution */
    int32_t pad_;
    float scale[MFN_MAX_LEVELS];
    uint32_t res[MFN_MAX_LEVELS];
    uint32_t offset[MFN_MAX_LEVELS];
    uint32_t size[MFN_MAX_LEVELS];
    int32_t table_kind[MFN_MAX_LEVELS];
} mfnerf_grid_desc;

/* Encode points x (n,3) f32.  The kernel first normalises x' = (x - x_min) / x_range exactly as
 * NGP.density does in torch (networks.py:105: (x-xyz_min)/(xyz_max-xyz_min); pass 0, 1 for inputs
 * already in [0,1]^3).  table (n_entries*F) f16.  out (n, n_levels*F) f16 row-major.
 * n_dev (optional, device i32): live row count <= n (rows beyond it are skipped). */
int mfnerf_grid_encode_fw(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                          const mfnerf_grid_desc* desc, const void* table_f16, void* out_f16,
                          mfnerf_stream_t stream);

/* mfnerf_grid_encode_fw with a level-major output: out_planes (n_levels, plane_stride) half2, the
 * features of level l of point i at [l*plane_stride + i] (plane_stride >= n).  Work is split by
 * level over the 8 XCDs so each XCD's L2 holds only its levels' tables.  Every level needs
 * size >= 2 entries (the kernel gathers 8 B at a time): a level of one entry is MFN_ERR_INVALID
 * here, before any launch, while mfnerf_grid_encode_fw accepts it.  Entries of the planes at or
 * past min(n, *n_dev) are left untouched. */
int mfnerf_grid_encode_fw_planar(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                 const mfnerf_grid_desc* desc, const void* table_f16, void* out_planes,
                                 int64_t plane_stride, mfnerf_stream_t stream);

/* The encoding's gradient with respect to the points (tcnn's input gradient, Linear interpolation):
 * dL_dout (n, n_levels*F) f32 row-major (as mfnerf_field_bw writes dL_dfeat) -> dL_dx (n,3) f32 in
 * the units of x (the 1/x_range of the normalisation included); x, n, n_dev, x_min, x_range, desc and
 * table_f16 as mfnerf_grid_encode_fw (the fp16 table the forward read).  fp32 accumulation in a
 * fixed order (no atomics): the same bits on every run.  Rows at or past min(n, *n_dev) are left
 * untouched. */
int mfnerf_grid_encode_bw_input(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                const mfnerf_grid_desc* desc, const void* table_f16, const float* dL_dout,
                                float* dL_dx, mfnerf_stream_t stream);

/* mfnerf_grid_encode_bw_input reduced per ray (the backward of the ray march,
 * custom_functions.py:103-112, without the per-sample gradient in memory): for each row r of rays_a
 * (n_rays,3) i64 = (ray, first sample, samples), over the samples s of its segment of xyzs (n_samples,3),
 * ts (n_samples), dL_dfeat (n_samples, n_levels*F), dL_ddirs (n_samples,3):
 *     dL_drays_o[ray] = sum_s dL/dxyz_s,   dL_drays_d[ray] = sum_s (ts_s * dL/dxyz_s + dL_ddirs_s)
 * (both (n_rays,3) f32; a ray without samples gets zeros; a segment is clamped to n_samples).  One
 * wave per ray, a fixed summation order, no atomics: deterministic.  No allocation and no host read,
 * so it is legal inside stream capture. */
int mfnerf_rays_input_grad(const float* xyzs, const float* ts, const float* dL_dfeat, const float* dL_ddirs,
                           const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float x_min, float x_range,
                           const mfnerf_grid_desc* desc, const void* table_f16, float* dL_drays_o,
                           float* dL_drays_d, mfnerf_stream_t stream);

/* Scatter dL/dout (n, n_levels*F) f32 into grad_table (n_entries*F) f32.  workspace (optional,
 * mfnerf_grid_encode_bw_workspace() bytes, ZERO on the first call; the call leaves it zero again):
 * private copies of the dense coarse levels' gradient, which spread their hot-line atomics.
 * level_l1 == NULL: float atomics, ACCUMULATES into grad_table (caller zeroes).
 * level_l1 != NULL (device f32[n_levels] = mfnerf_grid_level_l1 of dL_dout, or any upper bound of
 * it): fixed-point accumulation -- int32 atomics of rint(v * 2^(30-e_l)), l1_l < 2^e_l, which cannot
 * overflow and run ~28% faster than float atomics on MI355X -- then converted back; grad_table must
 * be ZERO on entry and is OVERWRITTEN.  Resolution per level 2^(e_l-30) (~1e-9 of the level's L1). */
int64_t mfnerf_grid_encode_bw_workspace(const mfnerf_grid_desc* desc);
int mfnerf_grid_encode_bw(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                          const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, void* workspace,
                          const float* level_l1, mfnerf_stream_t stream);

/* mfnerf_grid_encode_bw in two calls (the scatter, then the fold of the private copies /
 * fixed-point conversion), so the scatter can be timed on its own and the finish scheduled later
 * (anything reading grad_table must come after the finish). */
int mfnerf_grid_encode_bw_scatter(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                  const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                  void* workspace, const float* level_l1, mfnerf_stream_t stream);
int mfnerf_grid_encode_bw_finish(const mfnerf_grid_desc* desc, float* grad_table, void* workspace,
                                 const float* level_l1, mfnerf_stream_t stream);

/* The fixed-point scatter (level_l1 required) by table partitions instead of memory-side atomics:
 * the hashed / shared tables are cut into partitions of up to 2048 entries; every (point, level,
 * corner row) becomes an 8-B record, sorted by partition in LDS and stored into fixed per-(partition,
 * work unit) slots, and one workgroup per partition sums its records exactly (int64 LDS atomics)
 * and stores the partition once, rounded to the same int32 fixed point as
 * mfnerf_grid_encode_bw_scatter (one rounding per entry).  parts: 1 = the dense coarse levels only
 * (atomics into the workspace's private copies, as mfnerf_grid_encode_bw_scatter), 2 = the
 * partitioned levels only, 3 = both.  The workspace prefix is the private copies, so
 * mfnerf_grid_encode_bw_finish / mfnerf_adam_step_fixed convert the result unchanged; grad_table must
 * be zero on entry before the partitioned tables (the levels added by atomics), and is overwritten
 * from there on.  workspace: mfnerf_grid_encode_bw_binned_workspace(desc, n_slots) bytes, zero on the
 * first call (the finish and the accumulate leave it zero); n_slots (0 or > n: n) is the live sample
 * count the record slots are sized for -- a training step passes its expected count, not its
 * capacity (rays x 1024 samples): a live count well above n_slots overflows slots, whose extra
 * records are added by integer atomics into the workspace's overflow words and from there into the
 * partition's sums (same sums, slower).  Bit-reproducible.  Replaces tcnn's hash-grid backward
 * scatter (networks.py:36-49 encoding, half2 atomics there). */
int64_t mfnerf_grid_encode_bw_binned_workspace(const mfnerf_grid_desc* desc, int64_t n_max);
/* Adam arguments for the fused partitioned accumulate (mfnerf_grid_encode_bw_binned_adam). */
typedef struct {
    float* params;            /* the flat f32 master parameters, Adam m and v, and the f16 mirror */
    float* m;
    float* v;
    void* p16;
    int64_t table_offset;     /* index of the grid table's first value in those vectors */
    float lr, beta1, beta2, eps;
    const int32_t* step_dev;  /* as mfnerf_adam_step_fixed */
    const float* lr_dev;
    const mfnerf_amp_state* amp;
} mfnerf_adam_fused;
int mfnerf_grid_encode_bw_binned(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                 const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                 void* workspace, int64_t n_slots, const float* level_l1, int parts,
                                 mfnerf_stream_t stream);
/* mfnerf_grid_encode_bw_binned (parts = 3) + mfnerf_grid_encode_bw_finish in float form for an
 * exchange before the optimizer (the data-parallel step): the accumulate writes the partitioned
 * tables' finished sums as floats (times 1 / the table's scale, as the finish would) and one finish
 * pass covers only the values before them.  Same floats as the two-call form.  grad_table must be
 * zero before the partitioned tables' first value (mfnerf_grid_binned_first_value); the rest is
 * overwritten.  Replaces tcnn's hash-grid backward (networks.py:36-49) feeding DDP's all-reduce
 * (train.py:284).  gate (optional, mfnerf_gate_wait): signalled once as the dense-level launch
 * starts (by its first workgroup; a signal launch when no dense-level launch runs).
 * flag (optional): mfnerf_flag_to_shards(grads, flag_world, flag_shard_len, flag) folded into the
 * finish pass, grad_table being grads + table_offset (the flat gradient's every value must be final
 * when this is enqueued; needs a non-empty table prefix before the partitioned tables). */
int mfnerf_grid_encode_bw_binned_float(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                       const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                       void* workspace, int64_t n_slots, const float* level_l1, int32_t* gate,
                                       const int32_t* flag, int64_t flag_world, int64_t flag_shard_len,
                                       int64_t table_offset, mfnerf_stream_t stream);
/* mfnerf_grid_encode_bw_binned (parts = 3) with the partitioned tables' Adam step fused into the
 * accumulate (adam: see mfnerf_adam_step_fixed_partial). */
int mfnerf_grid_encode_bw_binned_adam(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                      const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                      void* workspace, int64_t n_slots, const float* level_l1,
                                      const mfnerf_adam_fused* adam, mfnerf_stream_t stream);
/* The collective-free step's whole table-gradient + optimizer tail in three launches: the binned
 * scatter (parts = 3), an accumulate launch whose partitions apply Adam to the partitioned tables
 * (as mfnerf_grid_encode_bw_binned_adam) while its leading workgroups run mfnerf_adam_step_fixed's
 * update over [0, the partitioned tables' first value) -- the MLPs and the dense levels, whose
 * gradients are final before the scatter -- and a last small pass for the step's bookkeeping (step
 * count, GradScaler, level_l1 zeroed).  grads: the flat gradient of n_params values (the table's
 * at adam->table_offset), zero for the table on entry; step_dev / amp: adam's, writable.  Same bits
 * as mfnerf_grid_encode_bw_binned_adam + mfnerf_adam_step_fixed_partial (and as the unfused
 * mfnerf_grid_encode_bw_binned + mfnerf_adam_step_fixed).  packed (optional, else NULL): the last pass
 * also repacks the MLP weights from adam->p16 into the field head's fragment blob for rgb width
 * rgb_width (= mfnerf_field_pack_weights_f16(p16, p16 + 3072, rgb_width, packed), one launch less).
 * gate (optional, gate.hip's int32 {signals, waits, ticket}; NULL: none): a signal added as the
 * dense-level launch starts (round 4: the side stream's next march starts beside the scatter
 * without a signal kernel of its own).
 * Replaces tcnn's hash-grid backward + apex FusedAdam's step over the whole model (train.py:136). */
int mfnerf_grid_encode_bw_binned_adam_all(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                          const mfnerf_grid_desc* desc, const float* dL_dout, float* grads,
                                          int64_t n_params, void* workspace, int64_t n_slots, float* level_l1,
                                          const mfnerf_adam_fused* adam, int32_t* step_dev, mfnerf_amp_state* amp,
                                          void* packed, int rgb_width, int32_t* gate, mfnerf_stream_t stream);

/* out[l] += sum over rows i < n (or *n_dev) of |dL_dout[i][2l]| + |dL_dout[i][2l+1]| (f32). */
int mfnerf_grid_level_l1(const float* dL_dout, int64_t n, const int32_t* n_dev, int n_levels, float* out,
                         mfnerf_stream_t stream);


/* ---------------------------------------------------------------- NGP field head (MFMA) */

/* Weight blob for the two FullyFusedMLPs of NGP (networks.py:50-79) in this library's MFMA
 * fragment order (f16).  Built from fp32 tcnn-layout params by mfnerf_field_pack_weights. */
int64_t mfnerf_field_packed_bytes(int rgb_width);

/* params_xyz: (64*32 + 16*64) f32, row-major [out][in] per layer (tcnn layout, bias-free);
 * params_rgb: (W*32 + W*W + 16*W) f32.  Writes packed (mfnerf_field_packed_bytes). */
int mfnerf_field_pack_weights(const float* params_xyz, const float* params_rgb, int rgb_width, void* packed,
                              mfnerf_stream_t stream);

/* The same blob from the fp16 compute copy of the params (what packing the fp32 master gives). */
/* tcnn SphericalHarmonics degree 4 (networks.py:60-67 dir_encoder; input (d/|d| + 1)/2 as
 * networks.py:145-146 passes it): dirs01 (n, 3) f32 -> out (n, 16) f16.  The fused field head
 * computes the same encoding inside mfnerf_field_fw/bw; this is the tinycudann module route's. */
int mfnerf_sh4_fw(const float* dirs01, int64_t n, void* out_f16, mfnerf_stream_t stream);
int mfnerf_field_pack_weights_f16(const void* params_xyz_f16, const void* params_rgb_f16, int rgb_width, void* packed,
                                  mfnerf_stream_t stream);

/* NGP.forward (networks.py:134-155) on encoded features:
 *   h = xyz_mlp(feat); sigma = exp(h[0]); rgb = sigmoid(rgb_mlp([SH4((d/|d|+1)/2), h])).
 * feat: feat_plane_stride == 0 -> (n,32) f16 row-major (tcnn layout, mfnerf_grid_encode_fw);
 *       > 0 -> (16, feat_plane_stride) half2 level planes (mfnerf_grid_encode_fw_planar).
 * dirs (n,3) f32 (ignored when density_only) -> sigma (n) f32, rgb (n,3) f32. */
int mfnerf_field_fw(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
                    int rgb_width, int density_only, float* sigma, float* rgb, mfnerf_stream_t stream);
/* mfnerf_field_fw for the HDR model (NGP(rgb_act='None'), networks.py:134-155): the rgb head has no
 * output activation.  sigma as mfnerf_field_fw writes it (the same code up to the epilogue);
 * lograd_f16 (n,3) f16 = the head's three outputs rounded to half (tcnn's fp16 output), the input
 * format of the tonemap kernels.  Rows below min(n, *n_dev) are written. */
int mfnerf_field_fw_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                           const int32_t* n_dev, const void* packed, int rgb_width, float* sigma, void* lograd_f16,
                           mfnerf_stream_t stream);
/* The occupancy refresh's density query (networks.py:252-259, `density_grid_tmp[c, indices] =
 * self.density(xyzs)`): mfnerf_field_fw density_only over min(n, *n_dev) points, each sigma also
 * written to tmp[cell_idx[i]] (skipped for cell_idx < 0) -- the update's scatter in the same launch
 * (then call mfnerf_occupancy_update_dev with n_points = 0).  Duplicate cells: unordered, like
 * the reference's index_put; the engine's probes are distinct (mfnerf_occupancy_cells_unique). */
int mfnerf_field_fw_density_scatter(const void* feat_f16, int64_t feat_plane_stride, int64_t n, const int32_t* n_dev,
                                    const void* packed, int rgb_width, float* sigma, const int32_t* cell_idx,
                                    float* tmp, mfnerf_stream_t stream);

/* The whole test-time renderer in one persistent launch: rendering.py:46-118 (the progressive loop
 * over raymarching_test / the field / composite_test_fw) with its prologue, rendering.py:27-29 (the
 * ray/box test for ONE box, center and half_size (3) f32 on the device, and the near clamp).  Each
 * ray is marched (raymarching.cu:335-404, including the calc_dt(..., cascades) quirk; max_samples_dt
 * is calc_dt's 1024), encoded (mfnerf_grid_encode_fw's arithmetic on x' = (x - x_min) / x_range),
 * evaluated (mfnerf_field_fw, packed_weights from mfnerf_field_pack_weights, rgb_width 64 or 128)
 * and composited (volumerendering.cu:205-285, T a running product from 1) sample by sample until
 * T <= T_threshold, it leaves the box or ray_budget samples were evaluated.  No intermediate is
 * written to memory.  The grid must have n_levels * n_features == 32.
 * out: opacity, depth (n_rays), rgb (n_rays,3) f32 -- the un-blended sums (zeros for a ray that
 *      misses the box); samples (n_rays) i32, optional, the evaluated samples of each ray;
 *      total_samples (1) i64 = their sum.  queue (1) i32 is the launch's ray counter: it and
 *      total_samples are zeroed by the launch itself (a kernel), so a replayed graph needs no reset.
 * A ray's outputs do not depend on the rest of the batch.  n_rays == 0: nothing is launched. */
int mfnerf_render_test_fused(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                             const float* half_size, const uint8_t* bitfield, int cascades, float scale,
                             float exp_step_factor, int grid_size, int max_samples_dt, int ray_budget,
                             float T_threshold, float x_min, float x_range, const mfnerf_grid_desc* grid_desc,
                             const void* table_f16, const void* packed_weights, int rgb_width, int32_t* queue,
                             float* opacity, float* depth, float* rgb, int32_t* samples, int64_t* total_samples,
                             mfnerf_stream_t stream);

/* Backward of mfnerf_field_fw (recomputes the forward; same feat layouts).  dL_dsigma (n), dL_drgb (n,3) f32 ->
 * dL_dfeat (n,32) f32, and ADDS the weight grads into grad_xyz / grad_rgb (tcnn layout f32).
 * grad_scale: the loss scale -- factor applied to the incoming grads before the fp16 MFMA products
 * and removed from every output (keeps O(1e-6) per-sample grads out of the fp16 subnormals).
 * grad_scale == 0: the dynamic scale amp->scale, read on the device (amp required).
 * workspace: mfnerf_field_bw_workspace() bytes (per-workgroup weight-grad slab).
 * amp (optional): amp->nonfinite is set to 1 when any dL_dfeat or weight gradient is inf/nan (the
 * table gradient of mfnerf_grid_encode_bw is a weighted sum of dL_dfeat, so this flags the whole
 * step's gradient without scanning it; feeds mfnerf_adam_step's skip).
 * level_l1 (optional device f32[16], ACCUMULATED): the per-level L1 norm of dL_dfeat, i.e. what
 * mfnerf_grid_level_l1 computes, for free (the fixed-point scales of mfnerf_grid_encode_bw). */
int64_t mfnerf_field_bw_workspace(int64_t n, int rgb_width);
/* The weight-gradient slab rows field_bw writes into its workspace for rgb_width (the per-workgroup
 * partials mfnerf_field_bw_reduce folds); -1 for an unsupported width. */
int mfnerf_field_bw_slab_rows(int rgb_width);
int mfnerf_field_bw(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
                    int rgb_width, const float* dL_dsigma, const float* dL_drgb, float grad_scale, float* dL_dfeat,
                    float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                    mfnerf_stream_t stream);

/* mfnerf_field_bw plus the gradient with respect to the view directions: dL_ddirs (n,3) f32, rows
 * below min(n, *n_dev) written.  dL/dSH is rows 0..15 of the product d[SH;h] = Wr1^T dR1 the
 * backward forms anyway (fp16 operands, fp32 accumulation, the loss scale removed); the chain rule
 * through SH4 and the normalisation d/|d| is fp32, the forward's fp16 rounding of SH taken as the
 * identity.  Every other output is bit-identical to mfnerf_field_bw's, the deferred fold included;
 * a non-finite dL_ddirs raises amp->nonfinite as well.  With mfnerf_grid_encode_bw_input this is
 * tcnn's input gradient of the field (camera-pose refinement, train.py:91-94). */
int mfnerf_field_bw_inputs(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
                           int rgb_width, const float* dL_dsigma, const float* dL_drgb, float grad_scale, float* dL_dfeat,
                           float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                           float* dL_ddirs, mfnerf_stream_t stream);

/* mfnerf_field_bw / mfnerf_field_bw_inputs for the head without its sigmoid (mfnerf_field_fw_lograd):
 * dL_dlograd (n,3) f32 is the unscaled gradient with respect to the log-radiance, so the head's
 * output gradient is half(dL_dlograd * S) with no y(1-y) factor.  Everything else -- loss scale,
 * n_dev, slab and deferred fold, level_l1, the non-finite flag -- is mfnerf_field_bw's. */
int mfnerf_field_bw_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
                           int rgb_width, const float* dL_dsigma, const float* dL_dlograd, float grad_scale, float* dL_dfeat,
                           float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                           mfnerf_stream_t stream);
int mfnerf_field_bw_inputs_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
                                  int rgb_width, const float* dL_dsigma, const float* dL_dlograd, float grad_scale, float* dL_dfeat,
                                  float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                                  float* dL_ddirs, mfnerf_stream_t stream);

/* grad_xyz = grad_rgb = NULL in mfnerf_field_bw defers the weight-gradient fold: the per-block
 * partial sums stay in workspace (dL_dfeat, level_l1 and the data-gradient part of the non-finite
 * flag are complete when field_bw returns) and this call adds them into grad_xyz / grad_rgb in the
 * same fixed order (bit-identical to the undeferred call), raising nonfinite on an inf/nan weight
 * gradient.  The training step runs it on a second stream beside the table-gradient scatter, which
 * needs only dL_dfeat.  Part of the tcnn backward (networks.py:96-126) split for scheduling. */
int mfnerf_field_bw_reduce(int rgb_width, const void* workspace, float* grad_xyz, float* grad_rgb,
                           int32_t* nonfinite, mfnerf_stream_t stream);
/* mfnerf_field_bw_reduce STORING the folded sums (grad = fold, same order and bits) instead of adding
 * them: a gradient that holds only this step's weight gradient needs no zeroing first (the
 * data-parallel step, where nothing else adds into the MLPs' gradient). */
int mfnerf_field_bw_reduce_store(int rgb_width, const void* workspace, float* grad_xyz, float* grad_rgb,
                                 int32_t* nonfinite, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- standalone FullyFusedMLP (MFMA)
 * tinycudann.Network / NetworkWithInputEncoding's network as MF-NeRF configures them one module at a
 * time (models/networks.py:36-79, tcnn FullyFusedMLP: bias-free, ReLU, output activation None or
 * Sigmoid, fp16): what the reference's own networks.py runs when tinycudann is this library
 * (module swap).  n_in = 32, width 64 or 128, n_hidden_layers 1 or 2, n_out <= 16
 * (padded to 16 as tcnn does).  params: tcnn layout, row-major [out][in] per layer, f32. */
int64_t mfnerf_mlp_n_params(int n_in, int width, int n_hidden, int n_out);
int64_t mfnerf_mlp_packed_bytes(int n_in, int width, int n_hidden, int n_out);
int mfnerf_mlp_pack(const float* params, int n_in, int width, int n_hidden, int n_out, void* packed,
                    mfnerf_stream_t stream);
/* x (n, 32) f16 -> out (n, 16) f16 (columns >= n_out hold the padded outputs). */
int mfnerf_mlp_fw(const void* x_f16, int64_t n, const void* packed, int n_in, int width, int n_hidden, int n_out,
                  int output_sigmoid, void* out_f16, mfnerf_stream_t stream);
/* dout (n, 16) f16 (zero beyond n_out) -> dx (n, 32) f32 (written), grad (n_params f32, ADDED:
 * dW = dZ^T A summed over samples in a fixed chunk order).  workspace: mfnerf_mlp_bw_workspace bytes. */
int64_t mfnerf_mlp_bw_workspace(int64_t n, int n_in, int width, int n_hidden, int n_out);
int mfnerf_mlp_bw(const void* x_f16, int64_t n, const void* packed, int n_in, int width, int n_hidden, int n_out,
                  int output_sigmoid, const void* dout_f16, float* dx, float* grad, void* workspace,
                  mfnerf_stream_t stream);

/* ---------------------------------------------------------------- HDR tonemappers (exposure path)
 * The reference's --use_exposure model (networks.py:81-94,111-132): rgb_net's output is log-radiance,
 * and one tcnn.Network(1, 1, FullyFusedMLP ReLU/Sigmoid, 64 neurons, 1 hidden layer) per colour
 * channel maps log-radiance + log(exposure) to an LDR value.  params (C, 2048) f32: per channel
 * W1 (64,16) row-major, then W2 (16,64) row-major -- tcnn's layout with the scalar input padded to
 * 16, the padding holding ones (so b_j = sum_{k>=1} W1[j,k] is unit j's bias).  Per sample, channel:
 *     x16 = half(float(lograd) + log e),  h_j = half(relu(W1h[j,0]*x16 + b_j)),
 *     y = half(sigmoid(sum_j W2h[0,j]*h_j)),  weights rounded to half, fp32 accumulation
 * ("Tonemapper semantics").  C = 1 (one network: tcnn.Network.forward) or 3 (the
 * model's three in one launch); no padded (n,16) row exists in memory.
 * exposure: NULL = unit exposure (log e = 0); else device f32 read at [i * exposure_stride],
 * exposure_stride 0 (one value for all samples: the test path's scalar, train.py:102-103) or
 * 1 (per sample: the train path's repeat_interleave, rendering.py:142-144). */

/* networks.py:81-94,111-132 forward: lograd (n,C) f16 -> rgb (n,C) f16.  n = 0 is a no-op. */
int mfnerf_tonemap_fw(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t n, int C,
                      const float* params, void* rgb_f16, mfnerf_stream_t stream);
/* networks.py:81-94,111-132 backward workspace: one row of C*192 f32 sums per workgroup (any content). */
int64_t mfnerf_tonemap_bw_workspace(int64_t n, int C);
/* networks.py:81-94,111-132 backward, fp32 from the forward's fp16 points, no loss scale:
 * dz = dL_drgb*y*(1-y) from the saved rgb_f16, h_j recomputed and gated on h_j > 0.  Writes
 * dL_dlograd (n,C) f32 and OVERWRITES grad_params (C,2048) f32 (dW1 columns 1..15 all hold the bias
 * gradient, dW2 rows 1..15 are zero; n = 0 zeroes it).  No gradient to the exposure.  Per-workgroup
 * partial sums, then a second launch adds them in a fixed order: no atomics, the same bits every run. */
int mfnerf_tonemap_bw(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t n, int C,
                      const float* params, const void* rgb_f16, const float* dL_drgb, float* dL_dlograd,
                      float* grad_params, void* workspace, mfnerf_stream_t stream);

/* The pair as the fused training step runs it (C = 3): `cap` is a capacity that sizes the grid and
 * the workspace (mfnerf_tonemap_bw_workspace(cap, 3)); the live count is min(cap, *n_dev), read on the
 * device, and nothing past it is read or written.  rgb (cap,3) is f32 holding the half value (what
 * the compositing kernels read; mfnerf_field_fw's convention): the forward's output equals
 * mfnerf_tonemap_fw's converted to float, bit for bit, and dL_dlograd equals mfnerf_tonemap_bw's.
 * grad_params keeps the backward's properties (fixed-order sums, no atomics, workspace content
 * free, *n_dev == 0 zeroes it); its summation order is that of a `cap`-sized launch. */
int mfnerf_tonemap_fw_live(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t cap,
                           const int32_t* n_dev, const float* params, float* rgb, mfnerf_stream_t stream);
int mfnerf_tonemap_bw_live(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t cap,
                           const int32_t* n_dev, const float* params, const float* rgb, const float* dL_drgb,
                           float* dL_dlograd, float* grad_params, void* workspace, mfnerf_stream_t stream);
/* rendering.py:142-145 (exposure repeated per sample through rays_a): for every row r of rays_a
 * (n_rays,3) i64 = (ray, start, count), exposure_s[start .. start+count) = exposure_ray[ray], clipped
 * to min(cap, *n_dev) rows.  exposure_ray (n_rays) f32, exposure_s (cap) f32: the exposure, not its log. */
int mfnerf_expand_exposure(const float* exposure_ray, const int64_t* rays_a, int64_t n_rays, int64_t cap,
                           const int32_t* n_dev, float* exposure_s, mfnerf_stream_t stream);
/* train.py:172-177: the tonemappers at log-radiance 0 and unit exposure give y_c; the loss term is
 * mean_c 0.5 (y_c - unit_exposure_rgb)^2.  loss_out[c] (C f32) is STORED channel c's share, and the
 * gradient (dL/dy_c = (y_c - u)/C, through the backward's fp16 points) is ADDED to grad_params
 * (C,2048): run it after mfnerf_tonemap_bw*, which overwrites that gradient.  Deterministic.  amp
 * (optional): amp->nonfinite is raised when the summed gradient holds an inf/nan. */
int mfnerf_tonemap_unit_loss(const float* params, int C, float unit_exposure_rgb, float* grad_params, float* loss_out,
                             mfnerf_amp_state* amp, mfnerf_stream_t stream);
/* Adam for a small parameter group kept outside the flat parameter vector (the tonemappers), after
 * mfnerf_pose_step: one workgroup, n <= 2^20, its own device step counter (bumped by an update),
 * lr_dev (optional) overriding lr.  amp->nonfinite set: nothing is touched -- the flag is left for
 * the main optimizer call, which does the GradScaler bookkeeping and clears it. */
int mfnerf_side_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1,
                          float beta2, float eps, int32_t* step_dev, const float* lr_dev, const mfnerf_amp_state* amp,
                          mfnerf_stream_t stream);


/* ---------------------------------------------------------------- occupancy grid refresh */

/* Device-only NGP.update_density_grid (networks.py:157-271, called every 16 steps by
 * train.py:165-168).  Three calls per refresh:
 *   1. mfnerf_occupancy_cells: the cells to probe, as jittered world points.  warmup != 0: every
 *      cell of every cascade (get_all_cells, networks.py:157-166); else per cascade n_uniform
 *      uniform cells + n_uniform cells drawn uniformly among {density_grid > density_threshold}
 *      (sample_uniform_and_occupied_cells, networks.py:168-192; the occupied list is in
 *      ascending morton order like torch.nonzero, and an empty set yields cell_idx -1).
 *      Outputs xyzs (n,3) f32 and cell_idx (n) i32 = cascade*G^3 + morton, with
 *      n = mfnerf_occupancy_points(...).  Random draws: counter-based hash of (seed, call_index).
 *   2. the caller evaluates sigma at xyzs (mfnerf_grid_encode_fw + mfnerf_field_fw density_only).
 *   3. mfnerf_occupancy_update: tmp = 0; tmp[cell_idx] = sigmas; density_grid = where(grid < 0,
 *      grid, max(grid*decay, tmp)) (decay = clamp(decay^(1/count_grid), 0.1, 0.95) when count_grid
 *      is given: erode); thr = min(mean(grid[grid > 0]), density_threshold) (NaN when no cell is
 *      positive, as Python's min(nan, x)); packbits(grid, thr) into bitfield.
 * tmp: cascades*G^3 f32 scratch.  workspace: mfnerf_occupancy_workspace() bytes, shared by 1 and 3. */
int64_t mfnerf_occupancy_workspace(int cascades, int grid_size);
int64_t mfnerf_occupancy_points(int cascades, int grid_size, int64_t n_uniform, int warmup);
int mfnerf_occupancy_cells(const float* density_grid, int cascades, int grid_size, float scale, int64_t n_uniform,
                           int warmup, float density_threshold, uint64_t seed, uint64_t call_index, float* xyzs,
                           int32_t* cell_idx, void* workspace, mfnerf_stream_t stream);
/* mfnerf_occupancy_cells with the call index read from (and then advanced in) device memory, so a
 * captured refresh draws new cells on every replay: call_index_dev (uint64, device) = the value
 * mfnerf_occupancy_cells' call_index would have; the same draws for the same index. */
int mfnerf_occupancy_cells_dev(const float* density_grid, int cascades, int grid_size, float scale, int64_t n_uniform,
                               int warmup, float density_threshold, uint64_t seed, uint64_t* call_index_dev,
                               float* xyzs, int32_t* cell_idx, void* workspace, mfnerf_stream_t stream);
int mfnerf_occupancy_update(float* density_grid, const float* sigmas, const int32_t* cell_idx, int64_t n_points,
                            int cascades, int grid_size, float decay, const float* count_grid, float density_threshold,
                            float* tmp, uint8_t* bitfield, void* workspace, mfnerf_stream_t stream);
/* The same probe de-duplicated (what the engine's refresh runs): of all the draws above only one
 * sigma per cell can reach the grid (`density_grid_tmp[c, indices] = ...`, networks.py:259, an
 * index_put whose duplicate writes land in no defined order), so the draws only mark their cells and
 * ONE jittered point is produced per distinct drawn cell -- keyed by (seed, call, cell) -- in ascending
 * row-major cell order within a cascade (x fastest; cell_idx still holds the cascade * G^3 + morton
 * index; the warm-up's every cell: morton order); *count_dev receives their number (<= the capacity
 * mfnerf_occupancy_points_unique(...)).  The set of probed cells is exactly the set the plain call
 * with the same seed and call index draws.  Deterministic.  The workspace must be zero-filled before
 * its first use (the call leaves its byte map zeroed); cascades*G^3 must be a multiple of 16.
 * mfnerf_occupancy_update_dev: mfnerf_occupancy_update over the first min(n_points, *n_dev) points;
 * tmp_zero = 1 promises tmp is all-zero on entry and leaves it zero (no fill launch). */
int64_t mfnerf_occupancy_points_unique(int cascades, int grid_size, int64_t n_uniform, int warmup);
int mfnerf_occupancy_cells_unique(const float* density_grid, int cascades, int grid_size, float scale,
                                  int64_t n_uniform, int warmup, float density_threshold, uint64_t seed,
                                  uint64_t call_index, float* xyzs, int32_t* cell_idx, int32_t* count_dev,
                                  void* workspace, mfnerf_stream_t stream);
int mfnerf_occupancy_cells_unique_dev(const float* density_grid, int cascades, int grid_size, float scale,
                                      int64_t n_uniform, int warmup, float density_threshold, uint64_t seed,
                                      uint64_t* call_index_dev, float* xyzs, int32_t* cell_idx, int32_t* count_dev,
                                      void* workspace, mfnerf_stream_t stream);
int mfnerf_occupancy_update_dev(float* density_grid, const float* sigmas, const int32_t* cell_idx, int64_t n_points,
                                const int32_t* n_dev, int cascades, int grid_size, float decay, const float* count_grid,
                                float density_threshold, float* tmp, int tmp_zero, uint8_t* bitfield,
                                void* workspace, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- validation metrics */

/* The validation metrics of one rendered view against its ground truth (train.py:65-67, 198-237:
 * torchmetrics PeakSignalNoiseRatio(data_range=1) and StructuralSimilarityIndexMeasure(data_range=1),
 * logged as test/psnr and test/ssim).  pred, target (H*W, 3) f32, row-major pixels, rgb interleaved.
 * out (2) f64, device: out[0] = mse = mean((pred - target)^2) over all 3*H*W values (the reference's
 * PSNR is 10*log10(1/mse)); out[1] = ssim = the mean over the three channels and the pixels whose
 * 11x11 window lies inside the image (5 <= y <= H-6, 5 <= x <= W-6) of
 *     ((2 mp mt + c1)(2 spt + c2)) / ((mp^2 + mt^2 + c1)(sp2 + st2 + c2)),  c1 = 0.01^2, c2 = 0.03^2,
 * the moments taken under the separable Gaussian window g[k] ~ exp(-(k-5)^2 / (2*1.5^2)), k = 0..10,
 * normalised to sum 1 -- torchmetrics' value: it pads by reflection and crops the padded border
 * from the map before the mean.  Inputs fp32; every product, filter sum, the expression and both
 * reductions fp64 (E[x^2] - mu^2 cancels in fp32 on flat bright windows); pred == target gives exactly
 * {0, 1}.  Fixed summation order, no atomics: the same bits on every run.  workspace:
 * mfnerf_image_metrics_workspace(H, W) bytes, any contents.  H < 11 or W < 11: MFN_ERR_INVALID,
 * nothing is launched and out is untouched (the workspace query returns 0).  No allocation and no
 * host read: legal inside stream capture. */
int64_t mfnerf_image_metrics_workspace(int64_t H, int64_t W);
int mfnerf_image_metrics(const float* pred, const float* target, int64_t H, int64_t W, double* out,
                         void* workspace, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- viewer frames */

/* One whole view's rays from a camera pose (datasets/ray_utils.py:8-47 get_ray_directions plus
 * :50-70 get_rays, which show_gui.py:74-75 re-runs per frame).  K4 = (fx, fy, cx, cy), four HOST
 * floats read during the call; pose = a DEVICE pointer to the row-major (3,4) camera-to-world matrix,
 * read by the kernel, so a replayed graph sees the pose its buffer holds then.  Pixel i = v*W + u gets
 * the camera direction d = (((u - cx) + 0.5)/fx, ((v - cy) + 0.5)/fy, 1), IEEE fp32 divisions;
 *   rays_d[i] = d . R^T (row a: fma(1, R[a][2], fma(dy, R[a][1], dx*R[a][0]))),  rays_o[i] = pose[:, 3]
 * copied bit for bit.  out: rays_o, rays_d (W*H, 3) f32.  W*H outside 1..2^29, a null pointer or a
 * zero focal length: MFN_ERR_INVALID, nothing is launched. */
int mfnerf_camera_rays(const float* K4, const float* pose, int64_t W, int64_t H, float* rays_o, float* rays_d,
                       mfnerf_stream_t stream);

/* Workspace bytes of mfnerf_frame_finish (mode 1; a constant). */
int64_t mfnerf_frame_finish_workspace(void);
/* A rendered view's sums to a displayable frame (show_gui.py:90-99 render_cam's tail and the save
 * branch of train.py:220-226).  opacity, depth (n) and rgb (n,3) f32 are what mfnerf_render_test_fused
 * wrote: rgb BEFORE the background blend.  frame_u8 (n,3) u8, 4-byte aligned; frame_f32 (n,3) f32
 * optional (NULL: not written), the GUI's float texture.
 * mode 0, colour: c = rgb + bg*(1 - opacity), the fp32 expression of rendering.py:93-94 (bg: 1 for
 *   exp_step_factor == 0, else 0; bg = 0 leaves an already blended rgb as it is); frame_f32 = c;
 *   frame_u8 = (c*255).astype(uint8) of train.py:223 -- the fp32 product truncated toward zero --
 *   except where that cast is undefined or wraps: a product outside [0, 256) is clamped to [0, 255]
 *   and NaN gives 0.  Reads opacity and rgb only.
 * mode 1, depth: depth2img (train.py:48-53): mn, mx over the n depths, x = (depth - mn)/(mx - mn)
 *   (one IEEE fp32 division), k = uint8(x*255) as above, frame_u8 = TURBO[k] in R,G,B order (the
 *   table of csrc/turbo_table.hpp; the reference's cv2 returns B,G,R); frame_f32 = frame_u8/255
 *   (show_gui.py:99).  mx == mn (the reference divides 0 by 0): k = 0 everywhere.  Depths are taken
 *   to be finite.  Reads depth only.  workspace: mfnerf_frame_finish_workspace() bytes, 4-byte
 *   aligned, any contents: a first launch writes every word the second one reads (per-workgroup
 *   min / max, no atomics), so the same bits on every run.
 * n == 0 is a no-op; an unknown mode, n outside 0..2^29, a null pointer the mode reads or a
 * misaligned frame_u8 / workspace: MFN_ERR_INVALID, nothing is launched. */
int mfnerf_frame_finish(const float* opacity, const float* depth, const float* rgb, int64_t n, int mode, float bg,
                        void* workspace, uint8_t* frame_u8, float* frame_f32, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- mesh extraction */

/* A triangle mesh of the density field (test.ipynb, the "mesh" cell: model.density on an N^3 lattice,
 * then mcubes.marching_cubes(sigma, sigma_threshold) on the host).  Here the lattice stays on the
 * device and the surface is extracted by marching tetrahedra on the Kuhn split of every cell (six
 * tetrahedra around the body diagonal; csrc/mesh_table.hpp, generated; specification:
 * tests/mesh_ref.py) -- the same iso-surface, triangulated differently from mcubes.
 *
 * The lattice has nx x ny x nz points (resolution + 1 per axis, each >= 2, nx*ny*nz < 2^31), point
 * (x, y, z) at linear index (z*ny + y)*nx + x and at world position lo + i*((hi - lo)/(n - 1)) per
 * axis in fp32.  lo and hi are HOST arrays of 3 floats, read during the call.  A point is inside
 * when sigma > threshold (NaN outside, +inf inside).  Cells are indexed (z*(ny-1) + y)*(nx-1) + x.
 *
 * mfnerf_mesh_lattice_points (test.ipynb mesh cell: the xyz grid handed to model.density): the
 * world positions of lattice points first .. first+count as xyz (count, 3) f32, so that the density
 * is evaluated slab by slab (mfnerf_grid_encode_fw + mfnerf_field_fw density_only) and the lattice
 * never exists as coordinates or features. */
int mfnerf_mesh_lattice_points(const float* lo, const float* hi, int64_t nx, int64_t ny, int64_t nz, int64_t first,
                               int64_t count, float* xyz, mfnerf_stream_t stream);
/* test.ipynb mesh cell, first pass of the extraction: vcount (nx*ny*nz) u8 = the crossing edges each
 * lattice point owns (0..7: the edges to p + d, d in {0,1}^3 \ {0}, with exactly one end inside);
 * tcount ((nx-1)*(ny-1)*(nz-1)) u8 = the triangles of each cell (0..12). */
int mfnerf_mesh_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float threshold, uint8_t* vcount,
                      uint8_t* tcount, mfnerf_stream_t stream);
/* test.ipynb mesh cell, second pass: voff / toff are the EXCLUSIVE prefix sums (i32) of vcount /
 * tcount from the same sigma and threshold.  Writes vertices (V, 3) f32 (ordered by owner, then by
 * edge type 1..7; the vertex of a crossing edge is p0 + t*d, t = (threshold - s0)/(s1 - s0) clamped
 * to [0, 1], 0.5 when not finite), normals (V, 3) f32 (-grad sigma by central differences of the
 * lattice, interpolated with t and normalised; (0,0,0) for a zero or non-finite gradient) and faces
 * (F, 3) i32 (ordered by cell, tetrahedron, triangle; wound so that the normal points from inside to
 * outside).  The caller sizes the outputs from the counts' totals V and F (both < 2^31). */
int mfnerf_mesh_emit(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float threshold, const int32_t* voff,
                     const int32_t* toff, const float* lo, const float* hi, float* vertices, float* normals,
                     int32_t* faces, mfnerf_stream_t stream);

/* Mesh cleaning (csrc/mesh_clean.hip; specification: tests/mesh_clean_ref.py).  The reference leaves
 * floaters to the user (test.ipynb mesh cell: "tune these parameters until the whole object lies
 * tightly in range with little noise", "sigma_threshold controls the noise"); these entry points
 * remove them on the device.  Everywhere: faces (F, 3) i32 with indices in [0, V) -- a face with an
 * index outside that range is skipped by every kernel (it joins nothing, counts nowhere and is never
 * kept), so bad input cannot write out of bounds; 0 <= V, F < 2^31; V == 0 or F == 0 launches
 * nothing and leaves every output untouched.  Integer atomics only: each output is a pure function
 * of the inputs, the same bits on every run.
 *
 * mfnerf_mesh_components replaces the "little noise" tuning of the test.ipynb mesh cell by an exact
 * notion of a floater: two vertices are connected when a face holds both; labels (V) i32 = the
 * smallest vertex index of each vertex's component (a vertex in no face labels itself);
 * face_counts (V) i32 = at r the number of faces of the component labelled r, 0 at every other
 * index.  Lock-free union-find in labels, then a flatten and a count launch; no host read. */
int mfnerf_mesh_components(const int32_t* faces, int64_t V, int64_t F, int32_t* labels, int32_t* face_counts,
                           mfnerf_stream_t stream);
/* test.ipynb mesh cell ("little noise"), the choice of what stays: with max_count the largest face
 * count, the component labelled r is kept when count[r] > 0, count[r] >= min_faces and
 * (double)count[r] >= (double)min_fraction * (double)max_count (min_fraction in [0, 1], an fp32 value
 * widened); with largest_only != 0 only the component of the largest count, the smallest label among
 * equals.  labels and face_counts as mfnerf_mesh_components wrote them.  Writes vkeep (V) u8 and
 * fkeep (F) u8, 1 = kept (a face is kept with its component), and stats, DEVICE int64[3]:
 * [0] components, [1] components kept, [2] scratch.  The thresholds are computed on the device. */
int mfnerf_mesh_select(const int32_t* faces, int64_t V, int64_t F, const int32_t* labels, const int32_t* face_counts,
                       int64_t min_faces, float min_fraction, int64_t largest_only, uint8_t* vkeep, uint8_t* fkeep,
                       int64_t* stats, mfnerf_stream_t stream);
/* test.ipynb mesh cell ("little noise"), the cleaned mesh: a stable compaction.  voff (V) / foff (F)
 * i32 are the EXCLUSIVE prefix sums of vkeep / fkeep.  Kept vertex v goes to row voff[v] of
 * out_vertices / out_normals / out_colors ((V', 3) f32, copied bit for bit; colors and out_colors may
 * both be NULL), kept face f to row foff[f] of out_faces (F', 3) i32 with each index i replaced by
 * voff[i].  Precondition: flags from mfnerf_mesh_select on the same mesh (every vertex of a kept
 * face is kept).  The caller sizes the outputs from the scans' totals V' and F'. */
int mfnerf_mesh_compact(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                        int64_t V, int64_t F, const uint8_t* vkeep, const int32_t* voff, const uint8_t* fkeep,
                        const int32_t* foff, float* out_vertices, float* out_normals, float* out_colors,
                        int32_t* out_faces, mfnerf_stream_t stream);
/* test.ipynb mesh cell ("tune these parameters until the whole object lies tightly in range"): the
 * density lattice culled by the occupancy bitfield, in place.  sigma (nx*ny*nz) f32 on the lattice
 * of the mesh section above (lo, hi HOST arrays of 3 floats; the fp32 positions
 * lo + i*((hi - lo)/(n - 1)) of mfnerf_mesh_lattice_points).  A point with any |coordinate| > scale is
 * cleared; otherwise mip = the position's cascade (raymarching.cu:19-23), its cell that of the march
 * (raymarching.cu:205-220 without the dt term: there is no ray), and the point is cleared when bit
 * (mip*G^3 + morton) & 7 of byte (mip*G^3 + morton) >> 3 of bitfield (mfnerf_packbits' layout) is
 * clear.  Cleared means sigma = 0.0f, a finite value; other points keep their bits.  G = grid_size
 * must be a power of two <= 1024, cascades in [1, 32], bitfield_bytes >= cascades*G^3/8. */
int mfnerf_mesh_occupancy_mask(float* sigma, const float* lo, const float* hi, int64_t nx, int64_t ny, int64_t nz,
                               const uint8_t* bitfield, int64_t bitfield_bytes, int64_t cascades, int64_t grid_size,
                               float scale, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- training batch */

/* One training batch from GPU-resident images (datasets/base.py:22-35 + train.py:93-105 get_rays,
 * datasets/ray_utils.py:50-70): per ray an image index (uniform over n_img; with same_image one
 * index for the whole batch) and a pixel index (uniform over hw), then
 *   rays_o = c2w[:, 3], rays_d = directions[pix] @ c2w[:, :3]^T, rgb = images[img, pix].
 * images (n_img, hw, 3) f32, poses (n_img, 3, 4) f32, directions (hw, 3) f32 (camera frame).
 * out (3, n_rays, 3) f32 = [rays_o | rays_d | rgb]; img_idx / pix_idx (n_rays) i32 optional.
 * Draws: counter-based hash of (seed, call[0], ray); call (optional device u64[2], zero-initialised)
 * is call[0] = the draw counter, incremented by the launch (by its last workgroup, call[1] being the
 * arrival ticket, 0 between launches), so graph replays sample fresh batches. */
int mfnerf_sample_rays(const float* images, const float* poses, const float* directions, int64_t n_img, int64_t hw,
                       int64_t n_rays, int same_image, uint64_t seed, uint64_t* call, float* out, int32_t* img_idx,
                       int32_t* pix_idx, mfnerf_stream_t stream);

/* mfnerf_sample_rays (no index outputs) fused with the ray-march prologue of the engine's step:
 * hits_t (n_rays,2) = ray_aabb_intersect of each drawn ray with the one box (center, half_size),
 * max_hits 1 (intersection.cu:5-56), with the near clamp t1 in [0, near) -> near
 * (rendering.py:29), and noise (n_rays) ~ U[0,1) (custom_functions.py:83) from the same counter
 * hash as the draws.  One launch instead of sample + AABB + clamp + noise kernels. */
int mfnerf_sample_rays_prep(const float* images, const float* poses, const float* directions, int64_t n_img,
                            int64_t hw, int64_t n_rays, int same_image, uint64_t seed, uint64_t* call, float* out,
                            const float* center, const float* half_size, float near, float* hits_t, float* noise,
                            mfnerf_stream_t stream);

/* mfnerf_sample_rays_prep that also returns the draws: img_idx / pix_idx (n_rays) i32 (optional), the
 * image and pixel of every ray, which the pose gradient needs (train.py:91-94).  The same kernel: for
 * the same seed and call counter the same draws and the same bits as mfnerf_sample_rays_prep, and
 * the indices of mfnerf_sample_rays. */
int mfnerf_sample_rays_prep_idx(const float* images, const float* poses, const float* directions, int64_t n_img,
                                int64_t hw, int64_t n_rays, int same_image, uint64_t seed, uint64_t* call, float* out,
                                const float* center, const float* half_size, float near, float* hits_t, float* noise,
                                int32_t* img_idx, int32_t* pix_idx, mfnerf_stream_t stream);

/* mfnerf_sample_rays_prep_idx (img_idx / pix_idx optional, each may be null) that also draws the
 * batch's random background colour (--random_bg, rendering.py:153-161: one torch.rand(3) per render()
 * call) into bg (3 f32, device, required), in the same launch, so the colour belongs to the batch it
 * was drawn with.  Component c = (mix32(key + c * 0x9E3779B97F4A7C15) >> 8) * 2^-24, U[0,1) with 24
 * bits, key = splitmix64(splitmix64(seed ^ 0xA0761D6478BD642F) ^ call[0]) with call[0] read before the
 * launch advances it (a stream constant of its own): a function of seed and call[0] alone, not of
 * n_rays or same_image.  One thread stores it.  Every other output has the bits of
 * mfnerf_sample_rays_prep_idx for the same seed and counter. */
int mfnerf_sample_rays_prep_bg(const float* images, const float* poses, const float* directions, int64_t n_img,
                               int64_t hw, int64_t n_rays, int same_image, uint64_t seed, uint64_t* call, float* out,
                               const float* center, const float* half_size, float near, float* hits_t, float* noise,
                               int32_t* img_idx, int32_t* pix_idx, float* bg, mfnerf_stream_t stream);

/* ---------------------------------------------------------------- camera-pose refinement */

/* The reference's --optimize_ext (train.py:91-94, 122-139; datasets/ray_utils.py axisangle_to_R): image
 * i has a rotation offset dR[i] (axis-angle) and a translation offset dT[i]; its refined pose is
 * [R(dR[i]) @ R0[i] | t0[i] + dT[i]], R(w) = I + sin(t)/t K + (1 - cos t)/t^2 K^2, t = |w| + 1e-7, fp32.
 * A ray of image i and pixel p has rays_d = R(dR[i]) u, u = R0[i] @ directions[p], rays_o = t0[i] + dT[i].
 *
 * mfnerf_pose_grad: the batch's ray gradients reduced per image,
 *     grad_dT[i] = sum_r dL_drays_o[r],   grad_dR[i] = sum_r J(dR[i], u_r)^T dL_drays_d[r]
 * over the rays r with img_idx[r] == i, J the Jacobian of w -> R(w) u for that formula, guard included
 * (the gradient of |w| at 0 taken as 0: u x g there, as torch autograd gives); the derivatives of the
 * two coefficients are evaluated by their series under t = 0.25, where the closed forms cancel.
 * dL_drays_o / dL_drays_d (n_rays,3) f32, img_idx / pix_idx (n_rays) i32, poses (n_img,3,4) the BASE
 * poses, directions (hw,3), dR (n_img,3); grad_dR / grad_dT (n_img,3) f32: every row is written (zeros
 * for an image without a ray; a ray whose img_idx is outside [0, n_img) or pix_idx outside [0, hw)
 * counts nowhere).  One workgroup per image, fixed summation order, no float atomics: the same bits
 * on every run.  amp (optional): a non-finite output raises amp->nonfinite (never cleared here).  No
 * allocation and no host read: legal inside stream capture. */
int mfnerf_pose_grad(const float* dL_drays_o, const float* dL_drays_d, const int32_t* img_idx, const int32_t* pix_idx,
                     const float* poses, const float* directions, const float* dR, int64_t n_rays, int64_t n_img,
                     int64_t hw, float* grad_dR, float* grad_dT, mfnerf_amp_state* amp, mfnerf_stream_t stream);

/* The pose optimizer (train.py:139: torch Adam over [dR, dT], betas 0.9/0.999, eps 1e-8, lr 1e-6) and
 * the composition of the refined poses.  dR, dT (n_img,3) f32 updated in place from grad_dR / grad_dT;
 * m, v (2,n_img,3) f32 = [dR's | dT's] moments; step_dev (device i32): completed pose steps, the
 * update uses t = *step_dev + 1 (bias corrections 1 - beta^t) and then increments it; lr_dev (optional
 * device f32) replaces lr.  Every row is updated (dense parameters: a zero gradient still decays the
 * moments and moves the row).  Then poses_out (n_img,3,4) f32 = [R(dR[i]) @ R0[i] | t0[i] + dT[i]] from
 * the base `poses` (poses_out != poses); with dR = dT = 0 it equals the base poses bit for bit.
 * amp (optional): when amp->nonfinite != 0 on entry (raised by mfnerf_field_bw or mfnerf_pose_grad)
 * dR, dT, m, v and step_dev stay untouched and poses_out is composed from the unchanged offsets;
 * nothing of amp is written -- the field's optimizer pass stays the one place that counts the skip
 * and runs GradScaler.update().  grad_dR == grad_dT == NULL: no update, the composition only. */
int mfnerf_pose_step(float* dR, float* dT, float* m, float* v, const float* grad_dR, const float* grad_dT,
                     const float* poses, int64_t n_img, float lr, float beta1, float beta2, float eps,
                     int32_t* step_dev, const float* lr_dev, const mfnerf_amp_state* amp, float* poses_out,
                     mfnerf_stream_t stream);

/* ---------------------------------------------------------------- optimizer */

/* Adam (apex FusedAdam semantics, adam_w_mode=False, no weight decay; train.py:136):
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr * (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps).
 * g is read as grad*grad_scale.  Optionally mirrors p into p_f16 (the fp16 compute copy).
 * step_dev (optional device i32): the number of completed steps; the update uses t = *step_dev+1
 * and the call then increments it (graph-replay safe).  Without step_dev, t = step.
 * lr_dev (optional device f32): learning rate read on the device (a schedule that does not
 * re-capture the graph); lr is used when it is NULL.
 * amp (optional): when amp->nonfinite != 0 the call changes nothing (params, m, v, p_f16 and
 * step_dev untouched) and increments amp->skipped -- torch GradScaler's skipped step on a
 * non-finite gradient (PL precision=16, train.py:287); amp->nonfinite is raised by
 * mfnerf_field_bw or mfnerf_check_finite.  Then GradScaler.update() (dynamic mode: backoff on a
 * skip, growth after growth_interval clean steps) and amp->nonfinite cleared -- done by the pass's
 * last workgroup (amp->ticket), no extra launch.
 * zero_grads != 0: grads is zeroed by the same pass (also on a skipped step), ready for the next
 * step's accumulation. */
int mfnerf_adam_step(float* params, float* grads, float* m, float* v, void* p_f16, int64_t n, float lr,
                     float beta1, float beta2, float eps, float grad_scale, int step, int32_t* step_dev,
                     const float* lr_dev, mfnerf_amp_state* amp, int zero_grads, mfnerf_stream_t stream);
/* The sharded update after the reduce-scatter (data parallel, train.py:277-287 DDP + apex
 * FusedAdam): mfnerf_flag_from_shard + mfnerf_adam_step(zero_grads = 0) in one launch.  The
 * non-finite flag is read from g_shard[0] (mfnerf_flag_to_shards put NaN there on any rank that
 * raised it; the reduction carries it to every shard); the last workgroup stores it in
 * amp->nonfinite for the bookkeeping, then zeroes zero[0, nz) (a per-step accumulator, e.g. the
 * grid's level L1 bounds).  amp and step_dev are required; g_shard is not modified. */
int mfnerf_adam_step_shard(float* params, const float* g_shard, float* m, float* v, void* p_f16, int64_t n, float lr,
                           float beta1, float beta2, float eps, float grad_scale, int32_t* step_dev, const float* lr_dev,
                           mfnerf_amp_state* amp, float* zero, int nz, mfnerf_stream_t stream);

/* mfnerf_grid_encode_bw_finish + mfnerf_adam_step (zero_grads on) in one pass, for a step with no
 * gradient exchange between them: grads[0, table_offset) are float gradients, grads[table_offset, ...)
 * the int32 fixed-point table sums mfnerf_grid_encode_bw_scatter left (level_l1 non-NULL there), the
 * dense prefix's in workspace's private copies.  Each value is converted exactly as the finish call
 * converts it and updated exactly as mfnerf_adam_step updates it (step_dev required, grad_scale 1);
 * grads and the private copies are zeroed (also on a skipped step).  n and table_offset: multiples
 * of 4, the table inside [table_offset, n).  level_l1 is zeroed after use, ready for the next step's
 * mfnerf_field_bw accumulation.  Replaces the two calls (and one pass over the gradient)
 * the reference makes as tcnn's backward + apex FusedAdam (train.py:136). */
int mfnerf_adam_step_fixed(float* params, float* grads, float* m, float* v, void* p_f16, int64_t n,
                           int64_t table_offset, const mfnerf_grid_desc* desc, void* workspace,
                           float* level_l1, float lr, float beta1, float beta2, float eps,
                           int32_t* step_dev, const float* lr_dev, mfnerf_amp_state* amp, mfnerf_stream_t stream);

/* The collective-free step's optimizer split in two (mfnerf_grid_encode_bw_binned_adam +
 * mfnerf_adam_step_fixed_partial): the partitioned accumulate applies Adam to the partitioned
 * tables' parameters itself, from each entry's finished int32 sum, and never writes their gradient
 * words (a record slot's overflow, added into them by atomics, is folded in and zeroed there); the
 * remaining pass updates [0, fused_from) only (fused_ovf non-NULL).  Same arithmetic, same bits as
 * the unsplit pair. */

int mfnerf_adam_step_fixed_partial(float* params, float* grads, float* m, float* v, void* p_f16, int64_t n,
                                   int64_t table_offset, const mfnerf_grid_desc* desc, void* workspace,
                                   float* level_l1, float lr, float beta1, float beta2, float eps,
                                   int32_t* step_dev, const float* lr_dev, mfnerf_amp_state* amp, int64_t fused_from,
                                   const int32_t* fused_ovf, mfnerf_stream_t stream);
/* value index (within the table) where the partitioned tables start, or -1 (nothing partitioned) */
int64_t mfnerf_grid_binned_first_value(const mfnerf_grid_desc* desc);
/* Values of the dense prefix (the leading own-table dense levels whose backward adds into private
 * copies and whose finish overwrites the gradient).  When it equals
 * mfnerf_grid_binned_first_value, mfnerf_grid_encode_bw_binned_float overwrites every table value
 * (no zeroing before it). */
int64_t mfnerf_grid_dense_values(const mfnerf_grid_desc* desc);
/* byte offset of the slot-overflow word inside the binned workspace sized for n_slots */
int64_t mfnerf_grid_encode_bw_binned_flag_offset(const mfnerf_grid_desc* desc, int64_t n_slots);

/* status[0] (device i32) = 1 if any of x (n f32, 16-byte aligned) is inf/nan, else 0 (a full scan;
 * the training step gets the same flag from mfnerf_field_bw's nonfinite argument instead). */
int mfnerf_check_finite(const float* x, int64_t n, int32_t* status, mfnerf_stream_t stream);

/* Sharded data parallel (mfnerf.dp.sharded_update): the step's non-finite flag rides the gradient
 * reduce-scatter.  mfnerf_flag_to_shards: if flag[0], grads[r*shard_len] = NaN for r < world (call
 * before the reduce-scatter); mfnerf_flag_from_shard: flag[0] = !isfinite(g_shard[0]) (after it).
 * Every rank then skips or updates together, with no extra collective. */
int mfnerf_flag_to_shards(float* grads, int64_t world, int64_t shard_len, const int32_t* flag, mfnerf_stream_t stream);
int mfnerf_flag_from_shard(const float* g_shard, int32_t* flag, mfnerf_stream_t stream);

/* A soft gate between two streams' captured graphs (no reference counterpart: it replaces the host
 * event the reference's PyTorch loop never needed, train.py:129-150 running one stream).  gate =
 * device int32[4] {signals, waits, -, timeouts}, zeroed once.  mfnerf_gate_signal adds a signal;
 * mfnerf_gate_wait (one thread) waits for the signal matching its own ticket, at most timeout_us,
 * then absorbs signals nobody waited for; a wait that gives up adds 1 to gate[3].
 * NO MEMORY ORDERING: signal and wait are relaxed atomics (an agent-scope release / acquire would
 * write back / invalidate the XCD's L2 on every poll), so the gate hands over no data -- a consumer
 * may not read anything the signaller wrote.  Ordering only: data hazards must be covered by stream
 * events, as the engine's are. */
int mfnerf_gate_signal(int32_t* gate, mfnerf_stream_t stream);
int mfnerf_gate_wait(int32_t* gate, int64_t timeout_us, mfnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MFNERF_H */
