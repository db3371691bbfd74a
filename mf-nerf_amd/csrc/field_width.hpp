// field_width.hpp -- the rgb widths the field head is built for, for the host code of field_fw.hip
// and field_bw.hip.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "../../include/mfnerf.h"

namespace mfn_field {

inline bool width_ok(int w) { return w == 64 || w == 128; }

inline int bad_width(int w) {
    mfn_set_error("field: rgb_width=%d unsupported (this build: 64 or 128)", w);
    return MFN_ERR_INVALID;
}

// f(std::integral_constant<int, W>{}) for a width that width_ok accepted: the one place that picks
// between the two instantiations (as mlp_dispatch in mlp.hip)
template <typename F>
auto width_dispatch(int rgb_width, F&& f) -> decltype(f(std::integral_constant<int, 64>{})) {
    if (rgb_width == 64) return f(std::integral_constant<int, 64>{});
    return f(std::integral_constant<int, 128>{});
}

}  // namespace mfn_field
