// cfx_ident.h — gfx950 kernels of the force-parameter identification (cfx_id_forces, cfx_id_normal).
//
// One thread per instance: single shooting from the rest state over N intervals x m sub-steps of Ding2003,
// Ding2007 or Hmed2018 (no fatigue), carrying the state (Cn, F) and its tangents d(Cn, F)/d theta in registers.
// The model constants are per-instance values here (theta[j * B + b], SoA), so the calcium row is integrated
// explicitly: the affine table of the callback kernels (cfx_kernels.h, integrate) bakes r0 = km_rest + r0_km in.
//
// Directions live in canonical slots, fixed per model, so every "which parameter is this direction" test is a
// compile-time one and a slot that a model does not have costs nothing:
//     slot   0        1        2          3     4     5     6    7
//     D03    a_rest   km_rest  tau1_rest  tau2
//     D07    a_scale  km_rest  tau1_rest  tau2  pd0   pdt
//     H18    a_rest   km_rest  tau1_rest  tau2  ar    bs    Is   cr
// D = 4 serves any subset of the first four, D = 8 everything else.  col[slot] is the caller's column of the slot
// (-1: not identified; its tangent is carried but never stored).  All col[] tests are wave-uniform.
//
// Stimulation sum (ding2003.py:200-252): r_i = 1 + (r0 - 1) e_i, e_i = exp(-(t_i - t_{i-1}) / tauc) (r_0 = 1), is
// affine in r0 = km_rest + r0_km, so with two theta-independent host tables per stage slot
//     cs(t) = c0[slot] + (r0 - 1) c1[slot],   c0 = sum_i exp(-(t - t_i) / tauc),  c1 = sum_{i>=1} e_i exp(-(t - t_i) / tauc)
// and d cs / d km_rest = c1[slot].  Hmed2018 weighs pulse i by lambda_i(theta, I_i); every exp(-(t - t_i) / tauc) of
// interval k factors as E[slot] w_i with E = exp(-(t - t_k) / tauc), w_i = exp(-(t_k - t_i) / tauc), hence
//     cs(t) = E[slot] (P0 + (r0 - 1) P1),  P0 = sum_i lambda_i w0[k][i],  P1 = sum_i lambda_i w1[k][i] (w1 = e_i w0):
// the per-pulse pair (w0, w1) is folded with lambda_i and its four partials once per interval, in a loop over the
// window that keeps no per-pulse register, whatever the truncation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfx_kernels.h"

namespace cfx {

enum { ID_A = 0, ID_KM, ID_TAU1, ID_TAU2, ID_P4, ID_P5, ID_P6, ID_P7, ID_SLOTS };

struct IdParams {
    int64_t B;       // instances
    int64_t n_data;  // 1: one experiment shared by every instance; B: one per instance
    int32_t N, m, T, Q;  // intervals, sub-steps, truncation, stage slots per interval (m * stages)
    int32_t n_id;
    int32_t col[ID_SLOTS];  // slot -> caller's parameter column (-1: constant def[slot])
    double def[ID_SLOTS];   // the handle's value of every slot
    double dt, h, inv_tauc, mult, r0_km;
    const double* c0;  // Ding: [N * Q]; Hmed: E [N * Q]
    const double* c1;  // Ding: [N * Q]
    const double* w0;  // Hmed: [N * T]
    const double* w1;  // Hmed: [N * T]
};

// slots a model has, and the ones its calcium state depends on
constexpr bool id_has(int model, int s) { return s < 4 || (model == M_D07 && s < 6) || model == M_H18; }
constexpr bool id_cn(int model, int s) { return s == ID_KM || (model == M_H18 && s >= 4); }
constexpr int id_slots(int model) { return model == M_D03 ? 4 : model == M_D07 ? 6 : 8; }

// Per-interval data of one thread: Ding2007 amplitude factor and its partials, Hmed forcing and its partials.
template <int D>
struct IdInterval {
    double E, dE4, dE5;  // D07: E(pw; pd0, pdt), dE/dpd0, dE/dpdt
    double G0, G[D];     // H18: cs = E[slot] G0, d cs / d slot = E[slot] G[slot]
};

// One right-hand side with tangents.  th: the instance's slot values; x = (cn, F), xd[r][s] = d x_r / d slot s.
template <int MODEL, int D>
__device__ __forceinline__ void id_rhs(const IdParams& P, const double (&th)[ID_SLOTS], const IdInterval<D>& iv,
                                       int q, double cn, double F, const double (&cnd)[D], const double (&Fd)[D],
                                       double& kcn, double& kF, double (&kcnd)[D], double (&kFd)[D]) {
    const double km = th[ID_KM], tau1 = th[ID_TAU1], tau2 = th[ID_TAU2];
    // calcium row (ding2003.py:254-266)
    double cs, csd_km;
    double e = 0.0;
    if constexpr (MODEL == M_H18) {
        e = P.c0[q];
        cs = e * iv.G0;
        csd_km = 0.0;
    } else {
        const double c1 = P.c1[q];
        cs = fma(km + P.r0_km - 1.0, c1, P.c0[q]);
        csd_km = c1;
    }
    kcn = P.inv_tauc * (cs - cn);
#pragma unroll
    for (int s = 0; s < D; ++s) {
        if (!id_has(MODEL, s) || !id_cn(MODEL, s)) {
            kcnd[s] = 0.0;
            continue;
        }
        const double csd = MODEL == M_H18 ? e * iv.G[s] : csd_km;
        kcnd[s] = P.inv_tauc * (csd - cnd[s]);
    }
    // force row (ding2003.py:274-311), partials as rhs_force (cfx_kernels.h) plus d / d tau2
    const double A = MODEL == M_D07 ? th[ID_A] * iv.E : th[ID_A];
    const double d1 = km + cn;
    const double d2 = fma(tau1, d1, tau2 * cn);
    const double R = frcp(d1 * d2);
    const double q1 = d2 * R;   // 1 / d1
    const double q2 = d1 * R;   // 1 / d2
    const double s1 = cn * q1;  // s
    const double t2 = d1 * q2;  // 1 / (tau1 + tau2 s)
    kF = P.mult * (A * s1 - F * t2);
    const double W0 = fma(A, q1 * q1, (F * tau2) * (q2 * q2));
    const double g_cn = P.mult * km * W0;
    const double g_F = -P.mult * t2;
    double ex[ID_SLOTS];
    ex[ID_A] = P.mult * s1 * (MODEL == M_D07 ? iv.E : 1.0);
    ex[ID_KM] = -cn * P.mult * W0;
    ex[ID_TAU1] = P.mult * F * (t2 * t2);
    ex[ID_TAU2] = P.mult * F * t2 * (cn * q2);
    const double gE = MODEL == M_D07 ? P.mult * s1 * th[ID_A] : 0.0;
    ex[ID_P4] = gE * iv.dE4;
    ex[ID_P5] = gE * iv.dE5;
    ex[ID_P6] = ex[ID_P7] = 0.0;
#pragma unroll
    for (int s = 0; s < D; ++s) {
        if (!id_has(MODEL, s)) {
            kFd[s] = 0.0;
            continue;
        }
        double t = g_F * Fd[s];
        if (id_cn(MODEL, s)) t = fma(g_cn, cnd[s], t);
        if (s < 4 || MODEL == M_D07) t += ex[s];
        kFd[s] = t;
    }
}

// Single shooting of instance b; node(k, F, Fd) is called at every node k = 0 .. N.
template <int MODEL, int SCHEME, int D, class NodeFn>
__device__ __forceinline__ void id_shoot(const IdParams& P, const double* __restrict__ theta,
                                         const double* __restrict__ U, int64_t b, NodeFn&& node) {
    constexpr int S = stages_of(SCHEME);
    const int64_t B = P.B;
    const int64_t ds = P.n_data, db = P.n_data == 1 ? 0 : b;  // data stride and column
    double th[ID_SLOTS];
#pragma unroll
    for (int s = 0; s < ID_SLOTS; ++s) {
        th[s] = P.def[s];
        if (id_has(MODEL, s) && P.col[s] >= 0) th[s] = theta[(int64_t)P.col[s] * B + b];
    }
    const double r0m1 = th[ID_KM] + P.r0_km - 1.0;
    const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0;
    double cn = 0.0, F = 0.0, cnd[D], Fd[D];
#pragma unroll
    for (int s = 0; s < D; ++s) cnd[s] = Fd[s] = 0.0;
    node(0, F, Fd);

    for (int k = 0; k < P.N; ++k) {
        IdInterval<D> iv;
        iv.E = 1.0;
        iv.dE4 = iv.dE5 = 0.0;
        iv.G0 = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) iv.G[s] = 0.0;
        if constexpr (MODEL == M_D07) {
            // ding2007.py:172-188: E = 1 - exp(-(pw - pd0) / pdt)
            const double pw = U[(int64_t)k * ds + db];
            const double ipdt = 1.0 / th[ID_P5];
            const double z = (pw - th[ID_P4]) * ipdt;
            const double ex = exp(-z);
            iv.E = 1.0 - ex;
            iv.dE4 = -ex * ipdt;
            iv.dE5 = -ex * z * ipdt;
        }
        if constexpr (MODEL == M_H18) {
            // hmed2018.py:169-180: lambda_i = ar (tanh(bs (I_i - Is)) + cr)
            const double ar = th[ID_P4], bs = th[ID_P5], Is = th[ID_P6], cr = th[ID_P7];
            double p0 = 0.0, p1 = 0.0, a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < P.T; ++i) {
                const double w0 = P.w0[(int64_t)k * P.T + i], w1 = P.w1[(int64_t)k * P.T + i];
                const double di = U[((int64_t)k * P.T + i) * ds + db] - Is;
                const double tnh = tanh(bs * di);
                const double sech2 = fma(-tnh, tnh, 1.0);
                const double lam = ar * (tnh + cr);
                const double dl[4] = {tnh + cr, ar * sech2 * di, -ar * bs * sech2, ar};
                p0 = fma(lam, w0, p0);
                p1 = fma(lam, w1, p1);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    a0[p] = fma(dl[p], w0, a0[p]);
                    a1[p] = fma(dl[p], w1, a1[p]);
                }
            }
            iv.G0 = fma(r0m1, p1, p0);
            if constexpr (D > ID_KM) iv.G[ID_KM] = p1;
            if constexpr (D == 8) {
#pragma unroll
                for (int p = 0; p < 4; ++p) iv.G[4 + p] = fma(r0m1, a1[p], a0[p]);
            }
        }
        const int q0 = k * P.Q;
        for (int j = 0; j < P.m; ++j) {
            const int q = q0 + j * S;
            double k1c, k1f, k1cd[D], k1fd[D];
            id_rhs<MODEL, D>(P, th, iv, q, cn, F, cnd, Fd, k1c, k1f, k1cd, k1fd);
            if constexpr (SCHEME == 1) {
                cn = cn + h * k1c;
                F = F + h * k1f;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    cnd[s] = cnd[s] + h * k1cd[s];
                    Fd[s] = Fd[s] + h * k1fd[s];
                }
            } else if constexpr (SCHEME == 2) {
                double xc = cn + h2 * k1c, xf = F + h2 * k1f, xcd[D], xfd[D];
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    xcd[s] = cnd[s] + h2 * k1cd[s];
                    xfd[s] = Fd[s] + h2 * k1fd[s];
                }
                double k2c, k2f, k2cd[D], k2fd[D];
                id_rhs<MODEL, D>(P, th, iv, q + 1, xc, xf, xcd, xfd, k2c, k2f, k2cd, k2fd);
                cn = cn + h * k2c;
                F = F + h * k2f;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    cnd[s] = cnd[s] + h * k2cd[s];
                    Fd[s] = Fd[s] + h * k2fd[s];
                }
            } else {
                double xc = cn + h2 * k1c, xf = F + h2 * k1f, xcd[D], xfd[D];
                double ac = k1c, af = k1f, acd[D], afd[D];
                double kc = 0.0, kf = 0.0, kcd[D], kfd[D];
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    acd[s] = k1cd[s];
                    afd[s] = k1fd[s];
                    xcd[s] = cnd[s] + h2 * k1cd[s];
                    xfd[s] = Fd[s] + h2 * k1fd[s];
                }
#pragma unroll
                for (int sg = 1; sg < 4; ++sg) {
                    id_rhs<MODEL, D>(P, th, iv, q + sg, xc, xf, xcd, xfd, kc, kf, kcd, kfd);
                    if (sg < 3) {
                        const double c = sg == 1 ? h2 : h;
                        ac = ac + 2.0 * kc;
                        af = af + 2.0 * kf;
                        xc = cn + c * kc;
                        xf = F + c * kf;
#pragma unroll
                        for (int s = 0; s < D; ++s) {
                            acd[s] = acd[s] + 2.0 * kcd[s];
                            afd[s] = afd[s] + 2.0 * kfd[s];
                            xcd[s] = cnd[s] + c * kcd[s];
                            xfd[s] = Fd[s] + c * kfd[s];
                        }
                    }
                }
                cn = cn + h6 * (ac + kc);
                F = F + h6 * (af + kf);
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    cnd[s] = cnd[s] + h6 * (acd[s] + kcd[s]);
                    Fd[s] = Fd[s] + h6 * (afd[s] + kfd[s]);
                }
            }
        }
        node(k + 1, F, Fd);
    }
}

// ---------------------------------------------------------------------------------------------------
// Node forces force[k * B + b], k = 0 .. N, and (SENS != nullptr) sens[(k * n_id + j) * B + b] = dF_k / d theta_j.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME, int D>
__global__ void __launch_bounds__(256) k_id_sens(const IdParams P, const double* __restrict__ theta,
                                                 const double* __restrict__ U, double* __restrict__ FORCE,
                                                 double* __restrict__ SENS) {
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    id_shoot<MODEL, SCHEME, D>(P, theta, U, b, [&](int k, double F, const double (&Fd)[D]) {
        FORCE[(int64_t)k * B + b] = F;
        if (SENS != nullptr) {
#pragma unroll
            for (int s = 0; s < D; ++s)
                if (id_has(MODEL, s) && P.col[s] >= 0) SENS[((int64_t)k * P.n_id + P.col[s]) * B + b] = Fd[s];
        }
    });
}

// ---------------------------------------------------------------------------------------------------
// Normal equations of the weighted least-squares fit, accumulated in registers over the nodes:
//   cost = dt sum_k w_k r_k^2 (r_k = F_k - y_k),  grad_j = 2 dt sum_k w_k r_k S_kj,
//   gn (packed lower triangle, i >= j at i (i + 1) / 2 + j) = 2 dt sum_k w_k S_ki S_kj.
// COST[b], GRAD[j * B + b], GN[p * B + b].  No atomics, no cross-thread reduction.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME, int D>
__global__ void __launch_bounds__(256) k_id_normal(const IdParams P, const double* __restrict__ theta,
                                                   const double* __restrict__ U, const double* __restrict__ Y,
                                                   const double* __restrict__ W, double* __restrict__ COST,
                                                   double* __restrict__ GRAD, double* __restrict__ GN) {
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t ds = P.n_data, db = P.n_data == 1 ? 0 : b;
    double cost = 0.0, g[D], H[D * (D + 1) / 2];
#pragma unroll
    for (int s = 0; s < D; ++s) g[s] = 0.0;
#pragma unroll
    for (int p = 0; p < D * (D + 1) / 2; ++p) H[p] = 0.0;
    id_shoot<MODEL, SCHEME, D>(P, theta, U, b, [&](int k, double F, const double (&Fd)[D]) {
        const double w = W[(int64_t)k * ds + db];
        const double r = F - Y[(int64_t)k * ds + db];
        const double wr = w * r;
        cost = fma(wr, r, cost);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            if (!id_has(MODEL, i)) continue;
            g[i] = fma(wr, Fd[i], g[i]);
            const double wi = w * Fd[i];
#pragma unroll
            for (int j = 0; j <= i; ++j)
                if (id_has(MODEL, j)) H[i * (i + 1) / 2 + j] = fma(wi, Fd[j], H[i * (i + 1) / 2 + j]);
        }
    });
    const double dt2 = 2.0 * P.dt;
    COST[b] = P.dt * cost;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (!id_has(MODEL, i) || P.col[i] < 0) continue;
        const int ci = P.col[i];
        GRAD[(int64_t)ci * B + b] = dt2 * g[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            if (!id_has(MODEL, j) || P.col[j] < 0) continue;
            const int cj = P.col[j];
            const int hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
            GN[(int64_t)(hi * (hi + 1) / 2 + lo) * B + b] = dt2 * H[i * (i + 1) / 2 + j];
        }
    }
}

hipError_t launch_id_sens(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                          double* force, double* sens, hipStream_t s);
hipError_t launch_id_normal(int model, int scheme, int d, const IdParams& P, const double* theta, const double* U,
                            const double* Y, const double* W, double* cost, double* grad, double* gn, hipStream_t s);

}  // namespace cfx
