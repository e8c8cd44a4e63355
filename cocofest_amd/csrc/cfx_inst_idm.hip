// Kernel instantiations of the multi-train force-parameter identification (cfx_idm.h): Ding2003, Ding2007 and
// Hmed2018 without fatigue, RK1 / RK2 / RK4, D = 4 (any subset of the four common parameters) or D = 8 direction
// slots, and the sum over the trains.
#include "cfx_idm.h"

namespace cfx {

namespace {

// Sum of the workspace WS [E][R][B] over the trains, in train order: row 0 -> COST [B], rows 1 .. n -> GRAD [n][B],
// the others -> GN, and (CPT != nullptr) cost_per_train [E][B].  One thread per (row, start): a fixed order, no
// atomics, no cross-lane arithmetic.
__global__ void __launch_bounds__(256) k_idm_reduce(int64_t B, int E, int R, int n, const double* __restrict__ WS,
                                                    double* __restrict__ COST, double* __restrict__ GRAD,
                                                    double* __restrict__ GN, double* __restrict__ CPT) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)blockIdx.y;
    if (b >= B) return;
    const bool cpt = r == 0 && CPT != nullptr;
    double acc = WS[(int64_t)r * B + b];
    if (cpt) CPT[b] = acc;
    for (int e = 1; e < E; ++e) {
        const double v = WS[((int64_t)e * R + r) * B + b];
        if (cpt) CPT[(int64_t)e * B + b] = v;
        acc = acc + v;
    }
    if (r == 0)
        COST[b] = acc;
    else if (r <= n)
        GRAD[(int64_t)(r - 1) * B + b] = acc;
    else
        GN[(int64_t)(r - 1 - n) * B + b] = acc;
}

struct SensArgs {
    const double* theta;
    double *force, *sens;
};
struct NormalArgs {
    const double* theta;
    double* ws;
};

dim3 grid_of(const IdmParams& P) { return dim3((unsigned)((P.B + kIdmBlock - 1) / kIdmBlock), (unsigned)P.E); }

template <int MODEL, int SCHEME, int D>
hipError_t run(const IdmParams& P, const SensArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_idm_sens<MODEL, SCHEME, D>), grid_of(P), dim3(kIdmBlock), 0, s, P, a.theta, a.force, a.sens);
    return hipGetLastError();
}
template <int MODEL, int SCHEME, int D>
hipError_t run(const IdmParams& P, const NormalArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_idm_normal<MODEL, SCHEME, D>), grid_of(P), dim3(kIdmBlock), 0, s, P, a.theta, a.ws);
    return hipGetLastError();
}

template <int MODEL, int D, class Args>
hipError_t by_scheme(int scheme, const IdmParams& P, const Args& a, hipStream_t s) {
    switch (scheme) {
        case 1: return run<MODEL, 1, D>(P, a, s);
        case 2: return run<MODEL, 2, D>(P, a, s);
        case 4: return run<MODEL, 4, D>(P, a, s);
        default: return hipErrorInvalidValue;
    }
}

template <class Args>
hipError_t dispatch(int model, int scheme, int d, const IdmParams& P, const Args& a, hipStream_t s) {
    if (d != 4 && d != 8) return hipErrorInvalidValue;
    switch (model) {
        case M_D03: return d == 4 ? by_scheme<M_D03, 4>(scheme, P, a, s) : hipErrorInvalidValue;
        case M_D07: return d == 4 ? by_scheme<M_D07, 4>(scheme, P, a, s) : by_scheme<M_D07, 8>(scheme, P, a, s);
        case M_H18: return d == 4 ? by_scheme<M_H18, 4>(scheme, P, a, s) : by_scheme<M_H18, 8>(scheme, P, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_idm_sens(int model, int scheme, int d, const IdmParams& P, const double* theta, double* force,
                           double* sens, hipStream_t s) {
    return dispatch(model, scheme, d, P, SensArgs{theta, force, sens}, s);
}

hipError_t launch_idm_normal(int model, int scheme, int d, const IdmParams& P, const double* theta, double* ws,
                             double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s) {
    const hipError_t e = dispatch(model, scheme, d, P, NormalArgs{theta, ws}, s);
    if (e != hipSuccess) return e;
    return launch_idm_reduce(P.B, P.E, P.n_id, ws, cost, grad, gn, cost_per_train, s);
}

hipError_t launch_idm_reduce(int64_t B, int E, int n, const double* ws, double* cost, double* grad, double* gn,
                             double* cost_per_train, hipStream_t s) {
    const int R = 1 + n + n * (n + 1) / 2;
    hipLaunchKernelGGL(k_idm_reduce, dim3((unsigned)((B + 255) / 256), (unsigned)R), dim3(256), 0, s, B, E, R, n, ws,
                       cost, grad, gn, cost_per_train);
    return hipGetLastError();
}

}  // namespace cfx
