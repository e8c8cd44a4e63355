// Kernel instantiations of the multi-train fatigue-parameter identification (cfx_idfm.h): Ding2003, Ding2007 and
// Hmed2018 with fatigue, RK1 / RK2 / RK4, four direction slots; the sum over the trains is cfx_idm.h's.
#include "cfx_idfm.h"
#include "cfx_id_launch.h"
#include "cfx_idm.h"

namespace cfx {

hipError_t launch_idfm_sens(int model, int scheme, const IdfmParams& P, const double* theta, double* force,
                            double* sens, hipStream_t s) {
    const dim3 grid = id_train_grid(P.B, P.E, kIdfmBlock);
    return idf_dispatch(model, scheme, [&](auto M, auto S) {
        hipLaunchKernelGGL((k_idfm_sens<M(), S()>), grid, dim3(kIdfmBlock), 0, s, P, theta, force, sens);
        return hipGetLastError();
    });
}

hipError_t launch_idfm_normal(int model, int scheme, const IdfmParams& P, const double* theta, double* ws,
                              double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s) {
    const dim3 grid = id_train_grid(P.B, P.E, kIdfmBlock);
    const hipError_t e = idf_dispatch(model, scheme, [&](auto M, auto S) {
        hipLaunchKernelGGL((k_idfm_normal<M(), S()>), grid, dim3(kIdfmBlock), 0, s, P, theta, ws);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return launch_idm_reduce(P.B, P.E, P.n_id, ws, cost, grad, gn, cost_per_train, s);
}

}  // namespace cfx
