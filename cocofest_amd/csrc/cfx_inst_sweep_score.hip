// Kernel instantiations of the scored stimulation-train sweep (cfx_sweep.h, k_sweep<MODEL, SCHEME, SCORE = true>):
// the six models x RK1 / RK2 / RK4.
#include "cfx_sweep.h"

namespace cfx {

namespace {

template <int MODEL, int SCHEME>
hipError_t run(const SweepParams& P, hipStream_t s) {
    dim3 grid((unsigned)((P.B + kSweepBlock - 1) / kSweepBlock));
    hipLaunchKernelGGL((k_sweep<MODEL, SCHEME, true>), grid, dim3(kSweepBlock), 0, s, P);
    return hipGetLastError();
}

template <int MODEL>
hipError_t by_scheme(int scheme, const SweepParams& P, hipStream_t s) {
    switch (scheme) {
        case 1: return run<MODEL, 1>(P, s);
        case 2: return run<MODEL, 2>(P, s);
        case 4: return run<MODEL, 4>(P, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_sweep_score(int model, int scheme, const SweepParams& P, hipStream_t s) {
    if (P.ty == nullptr || P.tn < 1 || P.metrics == nullptr) return hipErrorInvalidValue;
    switch (model) {
        case M_D03: return by_scheme<M_D03>(scheme, P, s);
        case M_D03F: return by_scheme<M_D03F>(scheme, P, s);
        case M_D07: return by_scheme<M_D07>(scheme, P, s);
        case M_D07F: return by_scheme<M_D07F>(scheme, P, s);
        case M_H18: return by_scheme<M_H18>(scheme, P, s);
        case M_H18F: return by_scheme<M_H18F>(scheme, P, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace cfx
