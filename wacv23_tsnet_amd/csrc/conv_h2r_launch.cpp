// conv_h2r_launch.cpp -- instantiations and launcher of the general implicit-GEMM convolution (conv_h2r.hpp).
#include <stdexcept>

#include "conv_h2r.hpp"
#include "kernels.hpp"

namespace tsnet {
namespace {

template <int KS, int BN, int NPROD, bool SMALL>
void go(const ConvArgs& a, hipStream_t s) {
    launch_tiles(a.in_alpha ? conv_h2r_kernel<KS, BN, 2, 2, NPROD, true, SMALL> : conv_h2r_kernel<KS, BN, 2, 2, NPROD, false, SMALL>, 256, (size_t)h2r_lds_bytes(a.Cin), a, s);
}

template <int NPROD>
void go_np(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    const bool small = a.Cin == 8;
    if (p.width == 128) {
        if (a.taps == 9 && !small) return go<3, 128, NPROD, false>(a, s);
    } else if (p.width == 64) {
        if (a.taps == 1 && !small) return go<1, 64, NPROD, false>(a, s);
        if (a.taps == 9) return small ? go<3, 64, NPROD, true>(a, s) : go<3, 64, NPROD, false>(a, s);
        if (a.taps == 49) return small ? go<7, 64, NPROD, true>(a, s) : go<7, 64, NPROD, false>(a, s);
    }
    plan_not_built(p, NPROD);
}

}  // namespace

void launch_conv_h2r(const ConvArgs& a, const ConvPlan& p, int nprod, hipStream_t s) {
    nprod == 3 ? go_np<3>(a, p, s) : (nprod == kNprodF16 ? go_np<kNprodF16>(a, p, s) : go_np<1>(a, p, s));
}

}  // namespace tsnet
