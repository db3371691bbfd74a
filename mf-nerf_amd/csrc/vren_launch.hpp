// vren_launch.hpp -- launch geometry shared by the vren_*.hip units only (the reference's `vren` op
// set, models/csrc/*.cu; their C-ABI entry points are in include/mfnerf.h).  Kernel arithmetic follows
// the reference statement by statement (see common.hpp for the fp contract); launch geometry and data
// flow are MI355X-first.
#pragma once
#include "common.hpp"

namespace mfn_vren {

// ray-level kernels use 64-thread workgroups (one wave) so a 8192-ray batch spreads over 128 CUs
// instead of 32 workgroups of 256
constexpr int RAY_BLOCK = 64;

inline unsigned blocks_for(int64_t n, int b) { return (unsigned)mfn::div_up<int64_t>(n, b); }

}  // namespace mfn_vren
