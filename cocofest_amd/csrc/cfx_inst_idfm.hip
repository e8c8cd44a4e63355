// Kernel instantiations of the multi-train fatigue-parameter identification (cfx_idfm.h): Ding2003, Ding2007 and
// Hmed2018 with fatigue, RK1 / RK2 / RK4, four direction slots; the sum over the trains is cfx_idm.h's.
#include "cfx_idfm.h"
#include "cfx_idm.h"

namespace cfx {

namespace {

struct SensArgs {
    const double* theta;
    double *force, *sens;
};
struct NormalArgs {
    const double* theta;
    double* ws;
};

dim3 grid_of(const IdfmParams& P) { return dim3((unsigned)((P.B + kIdfmBlock - 1) / kIdfmBlock), (unsigned)P.E); }

template <int MODEL, int SCHEME>
hipError_t run(const IdfmParams& P, const SensArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_idfm_sens<MODEL, SCHEME>), grid_of(P), dim3(kIdfmBlock), 0, s, P, a.theta, a.force, a.sens);
    return hipGetLastError();
}
template <int MODEL, int SCHEME>
hipError_t run(const IdfmParams& P, const NormalArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_idfm_normal<MODEL, SCHEME>), grid_of(P), dim3(kIdfmBlock), 0, s, P, a.theta, a.ws);
    return hipGetLastError();
}

template <int MODEL, class Args>
hipError_t by_scheme(int scheme, const IdfmParams& P, const Args& a, hipStream_t s) {
    switch (scheme) {
        case 1: return run<MODEL, 1>(P, a, s);
        case 2: return run<MODEL, 2>(P, a, s);
        case 4: return run<MODEL, 4>(P, a, s);
        default: return hipErrorInvalidValue;
    }
}

template <class Args>
hipError_t dispatch(int model, int scheme, const IdfmParams& P, const Args& a, hipStream_t s) {
    switch (model) {
        case M_D03F: return by_scheme<M_D03F>(scheme, P, a, s);
        case M_D07F: return by_scheme<M_D07F>(scheme, P, a, s);
        case M_H18F: return by_scheme<M_H18F>(scheme, P, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_idfm_sens(int model, int scheme, const IdfmParams& P, const double* theta, double* force,
                            double* sens, hipStream_t s) {
    return dispatch(model, scheme, P, SensArgs{theta, force, sens}, s);
}

hipError_t launch_idfm_normal(int model, int scheme, const IdfmParams& P, const double* theta, double* ws,
                              double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s) {
    const hipError_t e = dispatch(model, scheme, P, NormalArgs{theta, ws}, s);
    if (e != hipSuccess) return e;
    return launch_idm_reduce(P.B, P.E, P.n_id, ws, cost, grad, gn, cost_per_train, s);
}

}  // namespace cfx
