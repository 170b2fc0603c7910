// mmw_dispatch.hpp -- the launch layer's run-time choices as template arguments, host side only.  A launcher picks ONE
// instantiation with with_*; the prepare function of the same kernel family walks EVERY value with each_* and hands the
// instantiations to set_dynamic_lds -- both lists come from the value sets written here, so they cannot drift apart.
//     with_rows(rows_per_thread(cfg.max_pts), [&](auto R) { with_flag(f32, [&](auto F32) {
//         mmw_launch(k<decltype(R)::value, decltype(F32)::value>, ...); }); });
// The callback is a generic lambda; its argument is a std::integral_constant, so `decltype(R)::value` is a constant expression.
#pragma once

#include <hip/hip_runtime.h>
#include <initializer_list>
#include <type_traits>

#include "../../include/mmw.h"

namespace mmw {

// Rows (points) per thread of the kernels that take a scene's frame in ONE round of a 256-thread workgroup: 1, 2 or 4.
inline int rows_per_thread(int max_pts)
{
    static_assert(MMW_MAX_PTS_LIMIT <= 4 * 256, "k_normalize*, k_uart_read, k_track and k_scene take at most four rows per thread: a larger limit needs a round loop");
    return (max_pts + 255) / 256;
}

template <int V> using IntC = std::integral_constant<int, V>;

template <typename F> inline void with_rows(int r, F &&f) { if (r <= 1) f(IntC<1>{}); else if (r == 2) f(IntC<2>{}); else f(IntC<4>{}); }
template <typename F> inline void with_flag(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <typename F> inline void with_dx(int dx, F &&f) { if (dx == 9) f(IntC<9>{}); else f(IntC<6>{}); }

template <typename F> inline void each_rows(F &&f) { f(IntC<1>{}); f(IntC<2>{}); f(IntC<4>{}); }
template <typename F> inline void each_flag(F &&f) { f(std::false_type{}); f(std::true_type{}); }
template <typename F> inline void each_dx(F &&f) { f(IntC<9>{}); f(IntC<6>{}); }

// the dynamic LDS a kernel may be launched with (above 64 KiB the runtime wants to be told), a {kernel, bytes} row per kernel
struct KernelLds { const void *kernel; size_t bytes; };
inline hipError_t set_dynamic_lds(std::initializer_list<KernelLds> table)
{
    for (const KernelLds &t : table) {
        const hipError_t e = hipFuncSetAttribute(t.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mmw
