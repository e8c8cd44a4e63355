// Kernel instantiations of the fatigue-parameter identification (cfx_identf.h): Ding2003, Ding2007 and Hmed2018
// with fatigue, RK1 / RK2 / RK4, four direction slots.
#include "cfx_identf.h"
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

template <int MODEL, int SCHEME>
hipError_t run(const IdfParams& P, const SensArgs& a, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((k_idf_sens<MODEL, SCHEME>), grid, dim3(kBlock), 0, s, P, a.theta, a.U, a.force, a.sens);
    return hipGetLastError();
}
template <int MODEL, int SCHEME>
hipError_t run(const IdfParams& P, const NormalArgs& a, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((k_idf_normal<MODEL, SCHEME>), grid, dim3(kBlock), 0, s, P, a.theta, a.U, a.Y, a.W, a.cost,
                       a.grad, a.gn);
    return hipGetLastError();
}

template <int MODEL, class Args>
hipError_t by_scheme(int scheme, const IdfParams& P, const Args& a, hipStream_t s) {
    switch (scheme) {
        case 1: return run<MODEL, 1>(P, a, s);
        case 2: return run<MODEL, 2>(P, a, s);
        case 4: return run<MODEL, 4>(P, a, s);
        default: return hipErrorInvalidValue;
    }
}

template <class Args>
hipError_t dispatch(int model, int scheme, const IdfParams& P, const Args& a, hipStream_t s) {
    switch (model) {
        case M_D03F: return by_scheme<M_D03F>(scheme, P, a, s);
        case M_D07F: return by_scheme<M_D07F>(scheme, P, a, s);
        case M_H18F: return by_scheme<M_H18F>(scheme, P, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_idf_sens(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                           double* force, double* sens, hipStream_t s) {
    return dispatch(model, scheme, P, SensArgs{theta, U, force, sens}, s);
}

hipError_t launch_idf_normal(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                             const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s) {
    return dispatch(model, scheme, P, NormalArgs{theta, U, Y, W, cost, grad, gn}, s);
}

}  // namespace cfx
