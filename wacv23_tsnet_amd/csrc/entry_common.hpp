// entry_common.hpp -- what every C entry point of the library needs and nothing of the engine: how a HIP failure or a refused argument becomes
// an exception (HIP_TRY, ArgError / WeightError, check_launch), how the handle-free entries turn one into a status code and the text behind
// tsnet_op_last_error (OP_BEGIN / OP_END), and the grid of an elementwise launch.  Included by launch.hpp, op_entries.hpp and clip_entries.hpp, which are parts
// of engine.cpp's unit: everything here has internal linkage, as it had inside engine.cpp.  HOST code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/tsnet_abi.h"

namespace {

thread_local std::string g_op_error;    // the last refusal of a handle-free entry on this thread: tsnet_op_last_error

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            char buf__[512];                                                                        \
            snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            throw std::runtime_error(buf__);                                                        \
        }                                                                                           \
    } while (0)

struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct WeightError : std::runtime_error { using std::runtime_error::runtime_error; };
// f(), with a refusal of the planner or of a launcher (std::invalid_argument: conv_plan.hpp and the *_launch.cpp units know no ArgError)
// turned into the caller's ArgError, message kept
template <typename F>
inline auto arg_checked(F&& f) -> decltype(f()) {
    try { return f(); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
}

inline void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + " launch failed: " + hipGetErrorString(e));
}

inline int ew_grid(size_t total, int block = 256) {
    size_t g = (total + block - 1) / block;
    if (g > 256 * 8) g = 256 * 8;    // grid-stride above ~8 blocks per CU
    if (g < 1) g = 1;
    return (int)g;
}

// the body of a handle-free entry: ArgError -> TSNET_ERR_ARG, anything else -> TSNET_ERR_HIP, the text kept for tsnet_op_last_error
#define OP_BEGIN try {
#define OP_END                                                                   \
    } catch (const ArgError& e) { g_op_error = e.what(); return TSNET_ERR_ARG; }  \
      catch (const std::exception& e) { g_op_error = e.what(); return TSNET_ERR_HIP; } \
    return TSNET_OK;

}  // namespace
