// Kernel instantiations of the fatigue-parameter identification (cfx_identf.h): Ding2003, Ding2007 and Hmed2018
// with fatigue, RK1 / RK2 / RK4, four direction slots.
#include "cfx_identf.h"
#include "cfx_id_launch.h"
#include "cfx_launch.h"

namespace cfx {

hipError_t launch_idf_sens(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                           double* force, double* sens, hipStream_t s) {
    const dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    return idf_dispatch(model, scheme, [&](auto M, auto S) {
        hipLaunchKernelGGL((k_idf_sens<M(), S()>), grid, dim3(kBlock), 0, s, P, theta, U, force, sens);
        return hipGetLastError();
    });
}

hipError_t launch_idf_normal(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                             const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s) {
    const dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    return idf_dispatch(model, scheme, [&](auto M, auto S) {
        hipLaunchKernelGGL((k_idf_normal<M(), S()>), grid, dim3(kBlock), 0, s, P, theta, U, Y, W, cost, grad, gn);
        return hipGetLastError();
    });
}

}  // namespace cfx
