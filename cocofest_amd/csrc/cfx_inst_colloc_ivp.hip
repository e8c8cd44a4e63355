// Implicit collocation integrator instantiations (cfx_colloc_ivp.h): all models, degrees 1..5 compile-time, any other
// degree the generic LDS body; Hmed truncation buckets as in cfx_inst_hmed.hip.
#include "cfx_colloc_ivp.h"
#include "cfx_launch.h"

namespace cfx {

template <int MODEL, int TMAX, int DEG>
static hipError_t civp_deg(const KParams& P, const double* TB, const double* X0, const double* U, double* TR,
                           int32_t* ST, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kCivpBlock - 1) / kCivpBlock));
    hipLaunchKernelGGL((k_colloc_ivp<MODEL, TMAX, DEG>), grid, dim3(kCivpBlock), 0, s, P, TB, X0, U, TR, ST);
    return hipGetLastError();
}

template <int MODEL, int TMAX>
static hipError_t civp_t(const KParams& P, const double* TB, const double* X0, const double* U, double* TR,
                         int32_t* ST, hipStream_t s) {
    switch (P.deg) {
        case 1: return civp_deg<MODEL, TMAX, 1>(P, TB, X0, U, TR, ST, s);
        case 2: return civp_deg<MODEL, TMAX, 2>(P, TB, X0, U, TR, ST, s);
        case 3: return civp_deg<MODEL, TMAX, 3>(P, TB, X0, U, TR, ST, s);
        case 4: return civp_deg<MODEL, TMAX, 4>(P, TB, X0, U, TR, ST, s);
        case 5: return civp_deg<MODEL, TMAX, 5>(P, TB, X0, U, TR, ST, s);
        default: return civp_deg<MODEL, TMAX, 0>(P, TB, X0, U, TR, ST, s);
    }
}

template <int MODEL>
static hipError_t civp_hmed(int tmax, const KParams& P, const double* TB, const double* X0, const double* U,
                            double* TR, int32_t* ST, hipStream_t s) {
    switch (tmax) {
        case 4: return civp_t<MODEL, 4>(P, TB, X0, U, TR, ST, s);
        case 8: return civp_t<MODEL, 8>(P, TB, X0, U, TR, ST, s);
        case 16: return civp_t<MODEL, 16>(P, TB, X0, U, TR, ST, s);
        case 32: return civp_t<MODEL, 32>(P, TB, X0, U, TR, ST, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_colloc_ivp(int model, int tmax, const KParams& P, const double* TB, const double* X0,
                             const double* U, double* TR, int32_t* ST, hipStream_t s) {
    if (P.deg < 1 || P.deg > kMaxDeg) return hipErrorInvalidValue;
    switch (model) {
        case M_D03: return civp_t<M_D03, 1>(P, TB, X0, U, TR, ST, s);
        case M_D03F: return civp_t<M_D03F, 1>(P, TB, X0, U, TR, ST, s);
        case M_D07: return civp_t<M_D07, 1>(P, TB, X0, U, TR, ST, s);
        case M_D07F: return civp_t<M_D07F, 1>(P, TB, X0, U, TR, ST, s);
        case M_H18: return civp_hmed<M_H18>(tmax, P, TB, X0, U, TR, ST, s);
        case M_H18F: return civp_hmed<M_H18F>(tmax, P, TB, X0, U, TR, ST, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace cfx
