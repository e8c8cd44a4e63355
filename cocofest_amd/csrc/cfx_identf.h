// cfx_identf.h — gfx950 kernels of the fatigue-parameter identification (cfx_idf_forces, cfx_idf_normal).
//
// Step 2 of the identification protocol: the force parameters are fixed (the handle's constants) and the four
// fatigue parameters alpha_a, alpha_tau1, alpha_km, tau_fat are per-instance values (theta[j * B + b], SoA).  One
// thread per instance: single shooting from the fatigue rest state (0, 0, A_rest, tau1_rest, km_rest) over N
// intervals x m sub-steps of Ding2003 / Ding2007 / Hmed2018 WITH fatigue, carrying the five states and the tangents
// of (F, A, Tau1, Km) in registers.
//
// Directions live in canonical slots, one per parameter, so every "which parameter is this direction" test is a
// compile-time one:
//     slot   0         1            2          3
//            alpha_a   alpha_tau1   alpha_km   tau_fat
// col[slot] is the caller's column of the slot (-1: not identified; the slot's value is the handle's constant and its
// tangent is carried but never stored).  All col[] tests are wave-uniform.
//
// The calcium row has no tangent: r0 = km_rest + r0_km uses the CONSTANT km_rest with fatigue too
// (ding2003_with_fatigue.py: cn_sum_fun takes the model's km_rest, not the state Km), and the stimulation sum does not
// see theta.  It is integrated explicitly from the host tables of the force-parameter identification (cfx_ident.h),
// which depend on the stimulation rows only and are built on the first call:
//     Ding:  cs[slot] = c0[slot] + (r0 - 1) c1[slot]
//     Hmed:  cs[slot] = E[slot] G0,  G0 = sum_i lambda_i(I_i) (w0[k][i] + (r0 - 1) w1[k][i]) once per interval,
// lambda_i folded in a loop over the window that keeps no per-pulse register, whatever the truncation.
//
// Right-hand side (ding2003_with_fatigue.py:138-240; Ding2007: A E(pw) and A relaxing to a_scale; the force row in
// the single-reciprocal form of rhs_force, cfx_kernels.h, with its partials):
//     F'    = mult (A s - F d1 / d2),  s = cn / d1,  d1 = Km + cn,  d2 = Tau1 d1 + tau2 cn
//     A'    = alpha_a F - (A - A_rest) / tau_fat        d / d alpha_a = F,     d / d tau_fat = (A - A_rest) / tau_fat^2
//     Tau1' = alpha_tau1 F - (Tau1 - tau1_rest) / tau_fat      likewise along slots 1 and 3
//     Km'   = alpha_km F - (Km - km_rest) / tau_fat            likewise along slots 2 and 3
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfx_kernels.h"

namespace cfx {

enum { IDF_AA = 0, IDF_AT, IDF_AK, IDF_TF, IDF_SLOTS };
enum { IDF_NX = 5, IDF_NT = 4 };  // states; states that carry tangents (F, A, Tau1, Km = rows 1..4)

struct IdfParams {
    int64_t B;       // instances
    int64_t n_data;  // 1: one experiment shared by every instance; B: one per instance
    int32_t N, m, T, Q;  // intervals, sub-steps, truncation, stage slots per interval (m * stages)
    int32_t n_id;
    int32_t col[IDF_SLOTS];  // slot -> caller's parameter column (-1: constant def[slot])
    double def[IDF_SLOTS];   // the handle's value of every slot
    double dt, h, inv_tauc, mult, r0m1;  // r0m1 = km_rest + r0_km - 1
    double a_rest, tau1_rest, km_rest, tau2;  // a_rest: a_scale for Ding2007
    double pd0, pdt, ar, bs, Is, cr;
    const double* c0;  // Ding: [N * Q]; Hmed: E [N * Q]
    const double* c1;  // Ding: [N * Q]
    const double* w0;  // Hmed: [N * T]
    const double* w1;  // Hmed: [N * T]
};

// The instance's parameters and what the right-hand side needs of the interval.
struct IdfInstance {
    double aa, at, ak, itf, itf2;  // alpha_a, alpha_tau1, alpha_km, 1 / tau_fat, 1 / tau_fat^2
    double E;                      // D07: E(pw) of the interval
    double G0;                     // H18: cs = E[slot] G0
};

// One right-hand side with tangents.  x = (cn, F, A, Tau1, Km); xd[r][s] = d x_{r+1} / d slot s.
template <int MODEL>
__device__ __forceinline__ void idf_rhs(const IdfParams& P, const IdfInstance& I, int q, const double (&x)[IDF_NX],
                                        const double (&xd)[IDF_NT][IDF_SLOTS], double (&k)[IDF_NX],
                                        double (&kd)[IDF_NT][IDF_SLOTS]) {
    constexpr bool PW = MODEL == M_D07F;
    const double cn = x[0], F = x[1], A = x[2], tau1 = x[3], km = x[4];
    // calcium row (ding2003.py:254-266): no tangent
    const double cs = MODEL == M_H18F ? P.c0[q] * I.G0 : fma(P.r0m1, P.c1[q], P.c0[q]);
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

// y = x + c k on the states and the tangents
__device__ __forceinline__ void idf_axpy(double c, const double (&x)[IDF_NX], const double (&xd)[IDF_NT][IDF_SLOTS],
                                         const double (&k)[IDF_NX], const double (&kd)[IDF_NT][IDF_SLOTS],
                                         double (&y)[IDF_NX], double (&yd)[IDF_NT][IDF_SLOTS]) {
#pragma unroll
    for (int r = 0; r < IDF_NX; ++r) y[r] = x[r] + c * k[r];
#pragma unroll
    for (int r = 0; r < IDF_NT; ++r)
#pragma unroll
        for (int s = 0; s < IDF_SLOTS; ++s) yd[r][s] = xd[r][s] + c * kd[r][s];
}

// Single shooting of instance b; node(k, F, Fd) is called at every node k = 0 .. N.
template <int MODEL, int SCHEME, class NodeFn>
__device__ __forceinline__ void idf_shoot(const IdfParams& P, const double* __restrict__ theta,
                                          const double* __restrict__ U, int64_t b, NodeFn&& node) {
    constexpr int S = stages_of(SCHEME);
    const int64_t B = P.B;
    const int64_t ds = P.n_data, db = P.n_data == 1 ? 0 : b;  // data stride and column
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
    const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0;
    double x[IDF_NX] = {0.0, 0.0, P.a_rest, P.tau1_rest, P.km_rest}, xd[IDF_NT][IDF_SLOTS];
#pragma unroll
    for (int r = 0; r < IDF_NT; ++r)
#pragma unroll
        for (int s = 0; s < IDF_SLOTS; ++s) xd[r][s] = 0.0;
    node(0, x[1], xd[0]);

    for (int k = 0; k < P.N; ++k) {
        if constexpr (MODEL == M_D07F) {
            // ding2007.py:172-188: E = 1 - exp(-(pw - pd0) / pdt)
            const double pw = U[(int64_t)k * ds + db];
            I.E = 1.0 - exp(-(pw - P.pd0) / P.pdt);
        }
        if constexpr (MODEL == M_H18F) {
            // hmed2018.py:169-180: lambda_i = ar (tanh(bs (I_i - Is)) + cr)
            double g = 0.0;
            for (int i = 0; i < P.T; ++i) {
                const double w = fma(P.r0m1, P.w1[(int64_t)k * P.T + i], P.w0[(int64_t)k * P.T + i]);
                const double lam = P.ar * (tanh(P.bs * (U[((int64_t)k * P.T + i) * ds + db] - P.Is)) + P.cr);
                g = fma(lam, w, g);
            }
            I.G0 = g;
        }
        const int q0 = k * P.Q;
        for (int j = 0; j < P.m; ++j) {
            const int q = q0 + j * S;
            double k1[IDF_NX], k1d[IDF_NT][IDF_SLOTS];
            idf_rhs<MODEL>(P, I, q, x, xd, k1, k1d);
            if constexpr (SCHEME == 1) {
                idf_axpy(h, x, xd, k1, k1d, x, xd);
            } else if constexpr (SCHEME == 2) {
                double xs[IDF_NX], xsd[IDF_NT][IDF_SLOTS], k2[IDF_NX], k2d[IDF_NT][IDF_SLOTS];
                idf_axpy(h2, x, xd, k1, k1d, xs, xsd);
                idf_rhs<MODEL>(P, I, q + 1, xs, xsd, k2, k2d);
                idf_axpy(h, x, xd, k2, k2d, x, xd);
            } else {
                double xs[IDF_NX], xsd[IDF_NT][IDF_SLOTS], kk[IDF_NX], kkd[IDF_NT][IDF_SLOTS];
                idf_axpy(h2, x, xd, k1, k1d, xs, xsd);
#pragma unroll
                for (int sg = 1; sg < 4; ++sg) {
                    idf_rhs<MODEL>(P, I, q + sg, xs, xsd, kk, kkd);
                    if (sg < 3) {
                        idf_axpy(2.0, k1, k1d, kk, kkd, k1, k1d);  // k1 accumulates k1 + 2 k2 + 2 k3
                        idf_axpy(sg == 1 ? h2 : h, x, xd, kk, kkd, xs, xsd);
                    }
                }
                idf_axpy(1.0, k1, k1d, kk, kkd, k1, k1d);
                idf_axpy(h6, x, xd, k1, k1d, x, xd);
            }
        }
        node(k + 1, x[1], xd[0]);
    }
}

// ---------------------------------------------------------------------------------------------------
// Node forces force[k * B + b], k = 0 .. N, and (SENS != nullptr) sens[(k * n_id + j) * B + b] = dF_k / d theta_j.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME>
__global__ void __launch_bounds__(256) k_idf_sens(const IdfParams P, const double* __restrict__ theta,
                                                  const double* __restrict__ U, double* __restrict__ FORCE,
                                                  double* __restrict__ SENS) {
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    idf_shoot<MODEL, SCHEME>(P, theta, U, b, [&](int k, double F, const double (&Fd)[IDF_SLOTS]) {
        FORCE[(int64_t)k * B + b] = F;
        if (SENS != nullptr) {
#pragma unroll
            for (int s = 0; s < IDF_SLOTS; ++s)
                if (P.col[s] >= 0) SENS[((int64_t)k * P.n_id + P.col[s]) * B + b] = Fd[s];
        }
    });
}

// ---------------------------------------------------------------------------------------------------
// Normal equations of the weighted least-squares fit, accumulated in registers over the nodes (as k_id_normal):
//   cost = dt sum_k w_k r_k^2 (r_k = F_k - y_k),  grad_j = 2 dt sum_k w_k r_k S_kj,
//   gn (packed lower triangle, i >= j at i (i + 1) / 2 + j) = 2 dt sum_k w_k S_ki S_kj.
// COST[b], GRAD[j * B + b], GN[p * B + b].  No atomics, no cross-thread reduction.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME>
__global__ void __launch_bounds__(256) k_idf_normal(const IdfParams P, const double* __restrict__ theta,
                                                    const double* __restrict__ U, const double* __restrict__ Y,
                                                    const double* __restrict__ W, double* __restrict__ COST,
                                                    double* __restrict__ GRAD, double* __restrict__ GN) {
    constexpr int D = IDF_SLOTS;
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t ds = P.n_data, db = P.n_data == 1 ? 0 : b;
    double cost = 0.0, g[D], H[D * (D + 1) / 2];
#pragma unroll
    for (int s = 0; s < D; ++s) g[s] = 0.0;
#pragma unroll
    for (int p = 0; p < D * (D + 1) / 2; ++p) H[p] = 0.0;
    idf_shoot<MODEL, SCHEME>(P, theta, U, b, [&](int k, double F, const double (&Fd)[D]) {
        const double w = W[(int64_t)k * ds + db];
        const double r = F - Y[(int64_t)k * ds + db];
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
    const double dt2 = 2.0 * P.dt;
    COST[b] = P.dt * cost;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (P.col[i] < 0) continue;
        const int ci = P.col[i];
        GRAD[(int64_t)ci * B + b] = dt2 * g[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            if (P.col[j] < 0) continue;
            const int cj = P.col[j];
            const int hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
            GN[(int64_t)(hi * (hi + 1) / 2 + lo) * B + b] = dt2 * H[i * (i + 1) / 2 + j];
        }
    }
}

hipError_t launch_idf_sens(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                           double* force, double* sens, hipStream_t s);
hipError_t launch_idf_normal(int model, int scheme, const IdfParams& P, const double* theta, const double* U,
                             const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s);

}  // namespace cfx
