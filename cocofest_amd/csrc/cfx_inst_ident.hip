// Kernel instantiations of the force-parameter identification (cfx_ident.h): Ding2003, Ding2007 and Hmed2018
// without fatigue, RK1 / RK2 / RK4, D = 4 (any subset of the four common parameters) or D = 8 direction slots.
#include "cfx_ident.h"
#include "cfx_launch.h"

namespace cfx {

namespace {

struct SensArgs {
    const double *theta, *U;
    double *force, *sens;
};
struct NormalArgs {
    const double *theta, *U, *Y, *W;
    double *cost, *grad, *gn;
};

template <int MODEL, int SCHEME, int D>
hipError_t run(const IdParams& P, const SensArgs& a, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((k_id_sens<MODEL, SCHEME, D>), grid, dim3(kBlock), 0, s, P, a.theta, a.U, a.force, a.sens);
    return hipGetLastError();
}
template <int MODEL, int SCHEME, int D>
hipError_t run(const IdParams& P, const NormalArgs& a, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((k_id_normal<MODEL, SCHEME, D>), grid, dim3(kBlock), 0, s, P, a.theta, a.U, a.Y, a.W, a.cost,
                       a.grad, a.gn);
    return hipGetLastError();
}

template <int MODEL, int D, class Args>
hipError_t by_scheme(int scheme, const IdParams& P, const Args& a, hipStream_t s) {
    switch (scheme) {
        case 1: return run<MODEL, 1, D>(P, a, s);
        case 2: return run<MODEL, 2, D>(P, a, s);
        case 4: return run<MODEL, 4, D>(P, a, s);
        default: return hipErrorInvalidValue;
    }
}

template <class Args>
hipError_t dispatch(int model, int scheme, int d, const IdParams& P, const Args& a, hipStream_t s) {
    if (d != 4 && d != 8) return hipErrorInvalidValue;
    switch (model) {
        case M_D03: return d == 4 ? by_scheme<M_D03, 4>(scheme, P, a, s) : hipErrorInvalidValue;
        case M_D07: return d == 4 ? by_scheme<M_D07, 4>(scheme, P, a, s) : by_scheme<M_D07, 8>(scheme, P, a, s);
        case M_H18: return d == 4 ? by_scheme<M_H18, 4>(scheme, P, a, s) : by_scheme<M_H18, 8>(scheme, P, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_id_sens(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                          double* force, double* sens, hipStream_t s) {
    return dispatch(model, scheme, d, P, SensArgs{theta, U, force, sens}, s);
}

hipError_t launch_id_normal(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                            const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s) {
    return dispatch(model, scheme, d, P, NormalArgs{theta, U, Y, W, cost, grad, gn}, s);
}

}  // namespace cfx
