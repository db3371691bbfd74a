// grid_internal.hpp -- the launches that cross the hash-grid files.  Every kernel stays in its file's
// anonymous namespace; where another file starts one, the owning file gives it a plain host launcher.
// Hidden: none of them is part of the library's interface.
#pragma once
#include "common.hpp"

__global__ void mfn_bump_step_kernel(int32_t* s, mfnerf_amp_state* amp, float* zero, int nz);  // adam.hip

namespace mfn_grid {
#pragma GCC visibility push(hidden)

// grid_bw_atomic.hip: levels [0, l_first), l_first > 0, of a partitioned backward into the private
// copies `priv` -- grid_bw_dense_kernel where they all are dense own tables inside the copies, else
// grid_bw_kernel's request-shaped atomics.  zero_flag: cleared by the launch (NULL: none).  Returns
// whether the launch opens `gate` itself (the dense kernel does, given one; the atomics never).
bool launch_dense_levels(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                         const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, float* priv,
                         const float* level_l1, int l_first, int32_t* zero_flag, int32_t* gate,
                         mfnerf_stream_t stream);

// grid_bw_binned.hip: fold_convert_kernel over grad[0, total_vals) (flag NULL: no shard flag)
void launch_fold_convert(float* grad, int* priv, int64_t dense_vals, int64_t total_vals,
                         const mfnerf_grid_desc* desc, const float* level_l1, const int32_t* flag,
                         int64_t flag_world, int64_t flag_shard_len, int64_t table_off, mfnerf_stream_t stream);

#pragma GCC visibility pop
}  // namespace mfn_grid
