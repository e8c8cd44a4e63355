// Kernel instantiations of the multi-train force-parameter identification (cfx_idm.h): Ding2003, Ding2007 and
// Hmed2018 without fatigue, RK1 / RK2 / RK4, D = 4 (any subset of the four common parameters) or D = 8 direction
// slots, and the sum over the trains.
#include "cfx_idm.h"
#include "cfx_id_launch.h"

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

}  // namespace

hipError_t launch_idm_sens(int model, int scheme, int d, const IdmParams& P, const double* theta, double* force,
                           double* sens, hipStream_t s) {
    const dim3 grid = id_train_grid(P.B, P.E, kIdmBlock);
    return id_dispatch(model, scheme, d, [&](auto M, auto S, auto D) {
        hipLaunchKernelGGL((k_idm_sens<M(), S(), D()>), grid, dim3(kIdmBlock), 0, s, P, theta, force, sens);
        return hipGetLastError();
    });
}

hipError_t launch_idm_normal(int model, int scheme, int d, const IdmParams& P, const double* theta, double* ws,
                             double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s) {
    const dim3 grid = id_train_grid(P.B, P.E, kIdmBlock);
    const hipError_t e = id_dispatch(model, scheme, d, [&](auto M, auto S, auto D) {
        hipLaunchKernelGGL((k_idm_normal<M(), S(), D()>), grid, dim3(kIdmBlock), 0, s, P, theta, ws);
        return hipGetLastError();
    });
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
