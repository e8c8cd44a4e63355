// cfx_idfm.h — gfx950 kernels of the multi-train fatigue-parameter identification (cfx_idfm_forces, cfx_idfm_normal).
//
// E stimulation trains (recordings) share the four fatigue parameters alpha_a, alpha_tau1, alpha_km, tau_fat of every
// start; the force parameters are the handle's constants.  The fit minimises
//     sum_e dt_e sum_k w_{e,k} (F_{e,k}(theta) - y_{e,k})^2.
// Launch shape and train data are those of cfx_idm.h: one thread per (start b, train e), a grid of
// (ceil(B / 64), E) one-wave blocks, so every lane of a wave works on the same train and all train data is
// wave-uniform; SoA with the train as the minor index (times / act / value [P][E], counts [E], target / weight
// [Nmax + 1][E]); theta[j * B + b] per lane.
//
// The integration is that of cfx_identf.h: single shooting from the fatigue rest state (0, 0, A_rest, tau1_rest,
// km_rest) over the train's own N_e intervals x m sub-steps of Ding2003 / Ding2007 / Hmed2018 WITH fatigue, the five
// states and the tangents of (F, A, Tau1, Km) in the four canonical slots of cfx_identf.h, all in registers.  Every
// train starts from rest: a start state that depends on theta (a recording that begins fatigued) is not covered.
//
// The calcium row has no tangent (r0 = km_rest + r0_km uses the CONSTANT km_rest, the stimulation sum does not see
// theta), so its forcing is exactly cfx_sweep.h's, formed here from the train's pulses: at interval k the visible
// pulses are those with act <= k, the window the last `truncation` of them, and
//     G_k = sum_window r_i lambda_i exp(-(t_k - t_i) / tauc),   cs(t) = exp(-(t - t_k) / tauc) G_k,
// r_i = 1 for the window's first pulse, else 1 + (r0 - 1) exp(-(t_i - t_{i-1}) / tauc); lambda_i = 1 (Ding) or
// ar (tanh(bs (I_i - Is)) + cr) (Hmed2018).  G_k is ONE scalar folded once per interval in a loop that keeps no
// per-pulse register, so the truncation is unbounded; all exponents are <= 0.  An empty window gives cs = 0.
// Ding2007's interval uses A E(pw) with the width of the last visible pulse (the first one's before any is visible).
//
// No LDS, no atomics, no cross-lane arithmetic: the result of a (start, train) pair does not depend on its position
// in the batch or among the trains.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfx_identf.h"

namespace cfx {

struct IdfmParams {
    int64_t B;                  // starts
    int32_t E, P, Nmax, m;      // trains, pulse rows, node rows - 1, RK sub-steps per interval
    int32_t n_id;
    int32_t col[IDF_SLOTS];     // slot -> caller's parameter column (-1: constant def[slot])
    double def[IDF_SLOTS];      // the handle's value of every slot
    double inv_tauc, mult, r0m1, tau2;   // r0m1 = km_rest + r0_km - 1
    double a_rest, tau1_rest, km_rest;   // a_rest: a_scale for Ding2007
    double pd0, inv_pdt, ar, bs, Is, cr;
    const double* times;
    const int32_t* act;
    const double* value;
    const int32_t* n_pulses;
    const int32_t* truncation;
    const int32_t* n_shooting;
    const double* final_time;
    const double* target;
    const double* weight;
};

constexpr int kIdfmBlock = 64;  // one wave per block: a block is one train

// One right-hand side with tangents: idf_rhs (cfx_identf.h) with the calcium forcing cs given (idf_rhs reads it from
// the handle's tables and cannot be called here).  x = (cn, F, A, Tau1, Km); xd[r][s] = d x_{r+1} / d slot s; I.E is
// Ding2007's E(pw) of the interval.
template <int MODEL>
__device__ __forceinline__ void idfm_rhs(const IdfmParams& P, const IdfInstance& I, double cs,
                                         const double (&x)[IDF_NX], const double (&xd)[IDF_NT][IDF_SLOTS],
                                         double (&k)[IDF_NX], double (&kd)[IDF_NT][IDF_SLOTS]) {
    constexpr bool PW = MODEL == M_D07F;
    const double cn = x[0], F = x[1], A = x[2], tau1 = x[3], km = x[4];
    // calcium row (ding2003.py:254-266): no tangent
    k[0] = P.inv_tauc * (cs - cn);
    // force row, partials as rhs_force (cfx_kernels.h)
    const double Aeff = PW ? A * I.E : A;
    const double d1 = km + cn;
    const double d2 = fma(tau1, d1, P.tau2 * cn);
    const double R = frcp(d1 * d2);
    const double q1 = d2 * R;   // 1 / d1
    const double q2 = d1 * R;   // 1 / d2
    const double s1 = cn * q1;  // s
    const double t2 = d1 * q2;  // 1 / (tau1 + tau2 s)
    k[1] = P.mult * (Aeff * s1 - F * t2);
    const double W0 = fma(Aeff, q1 * q1, (F * P.tau2) * (q2 * q2));
    const double g_F = -P.mult * t2;
    const double g_A = P.mult * s1 * (PW ? I.E : 1.0);
    const double g_tau = P.mult * F * (t2 * t2);
    const double g_km = -cn * P.mult * W0;
    // fatigue rows
    const double dA = A - P.a_rest, dT = tau1 - P.tau1_rest, dK = km - P.km_rest;
    k[2] = I.aa * F - dA * I.itf;
    k[3] = I.at * F - dT * I.itf;
    k[4] = I.ak * F - dK * I.itf;
#pragma unroll
    for (int s = 0; s < IDF_SLOTS; ++s) {
        const double Fd = xd[0][s], Ad = xd[1][s], Td = xd[2][s], Kd = xd[3][s];
        kd[0][s] = fma(g_km, Kd, fma(g_tau, Td, fma(g_A, Ad, g_F * Fd)));
        double a = fma(I.aa, Fd, -I.itf * Ad);
        double t = fma(I.at, Fd, -I.itf * Td);
        double c = fma(I.ak, Fd, -I.itf * Kd);
        if (s == IDF_AA) a += F;
        if (s == IDF_AT) t += F;
        if (s == IDF_AK) c += F;
        if (s == IDF_TF) {
            a = fma(dA, I.itf2, a);
            t = fma(dT, I.itf2, t);
            c = fma(dK, I.itf2, c);
        }
        kd[1][s] = a;
        kd[2][s] = t;
        kd[3][s] = c;
    }
}

// Single shooting of start b on train e; node(k, F, Fd) is called at every node k = 0 .. N_e.  Returns N_e.
template <int MODEL, int SCHEME, class NodeFn>
__device__ __forceinline__ int idfm_shoot(const IdfmParams& P, const double* __restrict__ theta, int64_t b, int e,
                                          NodeFn&& node) {
    const int64_t B = P.B;
    const int E = P.E;
    const int np = P.n_pulses[e], T = P.truncation[e], N = P.n_shooting[e];
    const double dt = P.final_time[e] / (double)N;
    const double h = dt / (double)P.m, h2 = 0.5 * h, h6 = h / 6.0;
    const double eh2 = exp(-h2 * P.inv_tauc);
    double th[IDF_SLOTS];
#pragma unroll
    for (int s = 0; s < IDF_SLOTS; ++s) {
        th[s] = P.def[s];
        if (P.col[s] >= 0) th[s] = theta[(int64_t)P.col[s] * B + b];
    }
    IdfInstance I;
    I.aa = th[IDF_AA];
    I.at = th[IDF_AT];
    I.ak = th[IDF_AK];
    I.itf = 1.0 / th[IDF_TF];
    I.itf2 = I.itf * I.itf;
    I.E = 1.0;
    I.G0 = 0.0;
    double x[IDF_NX] = {0.0, 0.0, P.a_rest, P.tau1_rest, P.km_rest}, xd[IDF_NT][IDF_SLOTS];
#pragma unroll
    for (int r = 0; r < IDF_NT; ++r)
#pragma unroll
        for (int s = 0; s < IDF_SLOTS; ++s) xd[r][s] = 0.0;
    node(0, x[1], xd[0]);

    int nv = 0;  // visible pulses
    for (int k = 0; k < N; ++k) {
        while (nv < np && P.act[(int64_t)nv * E + e] <= k) ++nv;
        const int lo = nv > T ? nv - T : 0;
        const double tk = (double)k * dt;
        // the window's fold, as k_sweep (cfx_sweep.h)
        double G = 0.0, tprev = 0.0;
        for (int i = lo; i < nv; ++i) {
            const double ti = P.times[(int64_t)i * E + e];
            double w = i == lo ? 1.0 : fma(P.r0m1, exp(-(ti - tprev) * P.inv_tauc), 1.0);
            if constexpr (MODEL == M_H18F)  // hmed2018.py:169-180
                w *= P.ar * (tanh(P.bs * (P.value[(int64_t)i * E + e] - P.Is)) + P.cr);
            G = fma(w, exp(-(tk - ti) * P.inv_tauc), G);
            tprev = ti;
        }
        if constexpr (MODEL == M_D07F) {
            // ding2007.py:172-188, the width of the last visible pulse (the first one's before any is visible)
            if (np > 0) {
                const double pw = P.value[(int64_t)(nv > 0 ? nv - 1 : 0) * E + e];
                I.E = 1.0 - exp(-(pw - P.pd0) * P.inv_pdt);
            }
        }
        double ea = 1.0;  // exp(-(t - t_k) / tauc) at the start of the sub-step
        for (int j = 0; j < P.m; ++j) {
            double k1[IDF_NX], k1d[IDF_NT][IDF_SLOTS];
            idfm_rhs<MODEL>(P, I, ea * G, x, xd, k1, k1d);
            const double eb = exp(-((double)(j + 1) * h) * P.inv_tauc);
            if constexpr (SCHEME == 1) {
                idf_axpy(h, x, xd, k1, k1d, x, xd);
            } else if constexpr (SCHEME == 2) {
                double xs[IDF_NX], xsd[IDF_NT][IDF_SLOTS], k2[IDF_NX], k2d[IDF_NT][IDF_SLOTS];
                idf_axpy(h2, x, xd, k1, k1d, xs, xsd);
                idfm_rhs<MODEL>(P, I, (ea * eh2) * G, xs, xsd, k2, k2d);
                idf_axpy(h, x, xd, k2, k2d, x, xd);
            } else {
                const double cm = (ea * eh2) * G;
                double xs[IDF_NX], xsd[IDF_NT][IDF_SLOTS], kk[IDF_NX], kkd[IDF_NT][IDF_SLOTS];
                idf_axpy(h2, x, xd, k1, k1d, xs, xsd);
#pragma unroll
                for (int sg = 1; sg < 4; ++sg) {
                    idfm_rhs<MODEL>(P, I, sg < 3 ? cm : eb * G, xs, xsd, kk, kkd);
                    if (sg < 3) {
                        idf_axpy(2.0, k1, k1d, kk, kkd, k1, k1d);  // k1 accumulates k1 + 2 k2 + 2 k3
                        idf_axpy(sg == 1 ? h2 : h, x, xd, kk, kkd, xs, xsd);
                    }
                }
                idf_axpy(1.0, k1, k1d, kk, kkd, k1, k1d);
                idf_axpy(h6, x, xd, k1, k1d, x, xd);
            }
            ea = eb;
        }
        node(k + 1, x[1], xd[0]);
    }
    return N;
}

// ---------------------------------------------------------------------------------------------------
// Node forces force[(e * (Nmax + 1) + k) * B + b], k = 0 .. N_e, and (SENS != nullptr)
// sens[((e * (Nmax + 1) + k) * n_id + j) * B + b] = dF_{e,k} / d theta_j; NaN past the train's own N_e.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME>
__global__ void __launch_bounds__(kIdfmBlock) k_idfm_sens(const IdfmParams P, const double* __restrict__ theta,
                                                          double* __restrict__ FORCE, double* __restrict__ SENS) {
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = (int)blockIdx.y;
    if (b >= B) return;
    const int64_t row0 = (int64_t)e * (P.Nmax + 1);
    const int N = idfm_shoot<MODEL, SCHEME>(P, theta, b, e, [&](int k, double F, const double (&Fd)[IDF_SLOTS]) {
        FORCE[(row0 + k) * B + b] = F;
        if (SENS != nullptr) {
#pragma unroll
            for (int s = 0; s < IDF_SLOTS; ++s)
                if (P.col[s] >= 0) SENS[((row0 + k) * P.n_id + P.col[s]) * B + b] = Fd[s];
        }
    });
    const double nan = __builtin_nan("");
    for (int k = N + 1; k <= P.Nmax; ++k) {
        FORCE[(row0 + k) * B + b] = nan;
        if (SENS != nullptr)
            for (int j = 0; j < P.n_id; ++j) SENS[((row0 + k) * P.n_id + j) * B + b] = nan;
    }
}

// ---------------------------------------------------------------------------------------------------
// Normal equations of one (start, train) pair, accumulated in registers over the train's nodes with its own dt_e
// (the sums of k_idf_normal), written to the workspace WS [E][1 + n + n (n + 1) / 2][B]: row 0 the cost, rows 1 .. n
// the gradient, then the packed Gauss-Newton lower triangle, in the caller's columns.  The sum over the trains, in
// train order, follows in launch_idfm_normal.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME>
__global__ void __launch_bounds__(kIdfmBlock) k_idfm_normal(const IdfmParams P, const double* __restrict__ theta,
                                                            double* __restrict__ WS) {
    constexpr int D = IDF_SLOTS;
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = (int)blockIdx.y;
    if (b >= B) return;
    const int E = P.E;
    double cost = 0.0, g[D], H[D * (D + 1) / 2];
#pragma unroll
    for (int s = 0; s < D; ++s) g[s] = 0.0;
#pragma unroll
    for (int p = 0; p < D * (D + 1) / 2; ++p) H[p] = 0.0;
    idfm_shoot<MODEL, SCHEME>(P, theta, b, e, [&](int k, double F, const double (&Fd)[D]) {
        const double w = P.weight[(int64_t)k * E + e];
        const double r = F - P.target[(int64_t)k * E + e];
        const double wr = w * r;
        cost = fma(wr, r, cost);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            g[i] = fma(wr, Fd[i], g[i]);
            const double wi = w * Fd[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) H[i * (i + 1) / 2 + j] = fma(wi, Fd[j], H[i * (i + 1) / 2 + j]);
        }
    });
    const double dt = P.final_time[e] / (double)P.n_shooting[e], dt2 = 2.0 * dt;
    const int n = P.n_id;
    double* ws = WS + (int64_t)e * (1 + n + n * (n + 1) / 2) * B + b;
    ws[0] = dt * cost;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (P.col[i] < 0) continue;
        const int ci = P.col[i];
        ws[(int64_t)(1 + ci) * B] = dt2 * g[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            if (P.col[j] < 0) continue;
            const int cj = P.col[j];
            const int hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
            ws[(int64_t)(1 + n + hi * (hi + 1) / 2 + lo) * B] = dt2 * H[i * (i + 1) / 2 + j];
        }
    }
}

hipError_t launch_idfm_sens(int model, int scheme, const IdfmParams& P, const double* theta, double* force,
                            double* sens, hipStream_t s);
hipError_t launch_idfm_normal(int model, int scheme, const IdfmParams& P, const double* theta, double* ws,
                              double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s);

}  // namespace cfx
