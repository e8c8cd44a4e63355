// Kernel instantiations of the force-parameter identification (cfx_ident.h): Ding2003, Ding2007 and Hmed2018
// without fatigue, RK1 / RK2 / RK4, D = 4 (any subset of the four common parameters) or D = 8 direction slots.
#include "cfx_ident.h"
#include "cfx_id_launch.h"
#include "cfx_launch.h"

namespace cfx {

hipError_t launch_id_sens(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                          double* force, double* sens, hipStream_t s) {
    const dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    return id_dispatch(model, scheme, d, [&](auto M, auto S, auto D) {
        hipLaunchKernelGGL((k_id_sens<M(), S(), D()>), grid, dim3(kBlock), 0, s, P, theta, U, force, sens);
        return hipGetLastError();
    });
}

hipError_t launch_id_normal(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                            const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s) {
    const dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    return id_dispatch(model, scheme, d, [&](auto M, auto S, auto D) {
        hipLaunchKernelGGL((k_id_normal<M(), S(), D()>), grid, dim3(kBlock), 0, s, P, theta, U, Y, W, cost, grad, gn);
        return hipGetLastError();
    });
}

}  // namespace cfx
