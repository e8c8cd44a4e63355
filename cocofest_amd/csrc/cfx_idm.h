// cfx_idm.h — gfx950 kernels of the multi-train force-parameter identification (cfx_idm_forces, cfx_idm_normal).
//
// E stimulation trains share one parameter vector theta per start; the fit minimises
//     sum_e dt_e sum_k w_{e,k} (F_{e,k}(theta) - y_{e,k})^2.
// One thread per (start b, train e): the grid is (ceil(B / 64), E) one-wave blocks, so every lane of a wave works
// on the same train and all train data (pulse times, activation nodes, values, counts, target, weights) is
// wave-uniform, read at uniform addresses.  Train data is SoA with the train as the minor index:
//     times [P][E], act [P][E] (int32), value [P][E], n_pulses / truncation / n_shooting [E] (int32), final_time [E],
//     target / weight [Nmax + 1][E].
// theta is per lane, theta[j * B + b].  Single shooting from the rest state of Ding2003, Ding2007 or Hmed2018 (no
// fatigue) over the train's own N_e intervals x m sub-steps, carrying (Cn, F) and D tangent directions in registers,
// in the canonical slots of cfx_ident.h (D = 4 or 8).
//
// Calcium forcing with tangents, formed here with the semantics of cfx_sweep.h: at interval k the visible pulses are
// those with act <= k, the window the last `truncation` of them, r = 1 for the window's first pulse and
// r_i = 1 + (r0 - 1) e_i, e_i = exp(-(t_i - t_{i-1}) / tauc), otherwise.  The window is folded once per interval,
// anchored on t_k = k dt, in a loop that keeps no per-pulse register: with w_i = exp(-(t_k - t_i) / tauc)
//     G0 = sum lambda_i w_i,   G1 = sum_{i not first} lambda_i e_i w_i
// and for Hmed2018 the four partials of lambda_i (ar, bs, Is, cr; I_i) folded the same way into dG0, dG1.  Every
// stage is then, with E = exp(-(t - t_k) / tauc),
//     cs = E (G0 + (r0 - 1) G1),   d cs / d km_rest = E G1,   d cs / d lambda-slot = E (dG0 + (r0 - 1) dG1).
// All exponents are <= 0 (t_{i-1} <= t_i <= t_k <= t).  An empty window gives cs = 0.  Ding2007's interval uses the
// width of the last visible pulse (the first one's before any is visible).
//
// No LDS, no atomics, no cross-lane arithmetic: the result of a (start, train) pair does not depend on its position
// in the batch or among the trains.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfx_ident.h"

namespace cfx {

struct IdmParams {
    int64_t B;                  // starts
    int32_t E, P, Nmax, m;      // trains, pulse rows, node rows - 1, RK sub-steps per interval
    int32_t n_id;
    int32_t col[ID_SLOTS];      // slot -> caller's parameter column (-1: constant def[slot])
    double def[ID_SLOTS];       // the handle's value of every slot
    double inv_tauc, mult, r0_km;
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

constexpr int kIdmBlock = 64;  // one wave per block: a block is one train

// One right-hand side with tangents.  es: exp(-(t - t_k) / tauc) of the stage; iv.G0 = G0 + (r0 - 1) G1 and
// iv.G[slot] = d(that) / d slot, so cs = es iv.G0 for every model.  The force row and its partials are id_rhs's
// (cfx_ident.h), which reads its forcing from the handle's tables and cannot be called here.
template <int MODEL, int D>
__device__ __forceinline__ void idm_rhs(const IdmParams& P, const double (&th)[ID_SLOTS], const IdInterval<D>& iv,
                                        double es, double cn, double F, const double (&cnd)[D],
                                        const double (&Fd)[D], double& kcn, double& kF, double (&kcnd)[D],
                                        double (&kFd)[D]) {
    const double km = th[ID_KM], tau1 = th[ID_TAU1], tau2 = th[ID_TAU2];
    // calcium row (ding2003.py:254-266)
    kcn = P.inv_tauc * (es * iv.G0 - cn);
#pragma unroll
    for (int s = 0; s < D; ++s) {
        if (!id_has(MODEL, s) || !id_cn(MODEL, s)) {
            kcnd[s] = 0.0;
            continue;
        }
        kcnd[s] = P.inv_tauc * (es * iv.G[s] - cnd[s]);
    }
    // force row (ding2003.py:274-311), as id_rhs
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

// Single shooting of start b on train e; node(k, F, Fd) is called at every node k = 0 .. N_e.  Returns N_e.
template <int MODEL, int SCHEME, int D, class NodeFn>
__device__ __forceinline__ int idm_shoot(const IdmParams& P, const double* __restrict__ theta, int64_t b, int e,
                                         NodeFn&& node) {
    const int64_t B = P.B;
    const int E = P.E;
    const int np = P.n_pulses[e], T = P.truncation[e], N = P.n_shooting[e];
    const double dt = P.final_time[e] / (double)N;
    const double h = dt / (double)P.m, h2 = 0.5 * h, h6 = h / 6.0;
    const double eh2 = exp(-h2 * P.inv_tauc);
    double th[ID_SLOTS];
#pragma unroll
    for (int s = 0; s < ID_SLOTS; ++s) {
        th[s] = P.def[s];
        if (id_has(MODEL, s) && P.col[s] >= 0) th[s] = theta[(int64_t)P.col[s] * B + b];
    }
    const double r0m1 = th[ID_KM] + P.r0_km - 1.0;
    double cn = 0.0, F = 0.0, cnd[D], Fd[D];
#pragma unroll
    for (int s = 0; s < D; ++s) cnd[s] = Fd[s] = 0.0;
    node(0, F, Fd);

    int nv = 0;  // visible pulses
    for (int k = 0; k < N; ++k) {
        while (nv < np && P.act[(int64_t)nv * E + e] <= k) ++nv;
        const int lo = nv > T ? nv - T : 0;
        const double tk = (double)k * dt;
        IdInterval<D> iv;
        iv.E = 1.0;
        iv.dE4 = iv.dE5 = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) iv.G[s] = 0.0;
        {
            double g0 = 0.0, g1 = 0.0, tprev = 0.0;
            double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = lo; i < nv; ++i) {
                const double ti = P.times[(int64_t)i * E + e];
                const double w0 = exp(-(tk - ti) * P.inv_tauc);
                const double w1 = i == lo ? 0.0 : exp(-(ti - tprev) * P.inv_tauc) * w0;
                tprev = ti;
                if constexpr (MODEL == M_H18) {
                    // hmed2018.py:169-180: lambda_i = ar (tanh(bs (I_i - Is)) + cr)
                    const double ar = th[ID_P4], bs = th[ID_P5], Is = th[ID_P6], cr = th[ID_P7];
                    const double di = P.value[(int64_t)i * E + e] - Is;
                    const double tnh = tanh(bs * di);
                    const double lam = ar * (tnh + cr);
                    g0 = fma(lam, w0, g0);
                    g1 = fma(lam, w1, g1);
                    if constexpr (D == 8) {
                        const double sech2 = fma(-tnh, tnh, 1.0);
                        const double dl[4] = {tnh + cr, ar * sech2 * di, -ar * bs * sech2, ar};
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            a0[p] = fma(dl[p], w0, a0[p]);
                            a1[p] = fma(dl[p], w1, a1[p]);
                        }
                    }
                } else {
                    g0 = g0 + w0;
                    g1 = g1 + w1;
                }
            }
            iv.G0 = fma(r0m1, g1, g0);
            if constexpr (D > ID_KM) iv.G[ID_KM] = g1;
            if constexpr (MODEL == M_H18 && D == 8) {
#pragma unroll
                for (int p = 0; p < 4; ++p) iv.G[4 + p] = fma(r0m1, a1[p], a0[p]);
            }
        }
        if constexpr (MODEL == M_D07) {
            // ding2007.py:172-188: E = 1 - exp(-(pw - pd0) / pdt), the width of the last visible pulse
            if (np > 0) {
                const double pw = P.value[(int64_t)(nv > 0 ? nv - 1 : 0) * E + e];
                const double ipdt = 1.0 / th[ID_P5];
                const double z = (pw - th[ID_P4]) * ipdt;
                const double ex = exp(-z);
                iv.E = 1.0 - ex;
                iv.dE4 = -ex * ipdt;
                iv.dE5 = -ex * z * ipdt;
            }
        }
        double ea = 1.0;  // exp(-(t - t_k) / tauc) at the start of the sub-step
        for (int j = 0; j < P.m; ++j) {
            const double eb = exp(-((double)(j + 1) * h) * P.inv_tauc);
            double k1c, k1f, k1cd[D], k1fd[D];
            idm_rhs<MODEL, D>(P, th, iv, ea, cn, F, cnd, Fd, k1c, k1f, k1cd, k1fd);
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
                idm_rhs<MODEL, D>(P, th, iv, ea * eh2, xc, xf, xcd, xfd, k2c, k2f, k2cd, k2fd);
                cn = cn + h * k2c;
                F = F + h * k2f;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    cnd[s] = cnd[s] + h * k2cd[s];
                    Fd[s] = Fd[s] + h * k2fd[s];
                }
            } else {
                const double em = ea * eh2;
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
                    idm_rhs<MODEL, D>(P, th, iv, sg < 3 ? em : eb, xc, xf, xcd, xfd, kc, kf, kcd, kfd);
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
            ea = eb;
        }
        node(k + 1, F, Fd);
    }
    return N;
}

// ---------------------------------------------------------------------------------------------------
// Node forces force[(e * (Nmax + 1) + k) * B + b], k = 0 .. N_e, and (SENS != nullptr)
// sens[((e * (Nmax + 1) + k) * n_id + j) * B + b] = dF_{e,k} / d theta_j; NaN past the train's own N_e.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME, int D>
__global__ void __launch_bounds__(kIdmBlock) k_idm_sens(const IdmParams P, const double* __restrict__ theta,
                                                        double* __restrict__ FORCE, double* __restrict__ SENS) {
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = (int)blockIdx.y;
    if (b >= B) return;
    const int64_t row0 = (int64_t)e * (P.Nmax + 1);
    const int N = idm_shoot<MODEL, SCHEME, D>(P, theta, b, e, [&](int k, double F, const double (&Fd)[D]) {
        FORCE[(row0 + k) * B + b] = F;
        if (SENS != nullptr) {
#pragma unroll
            for (int s = 0; s < D; ++s)
                if (id_has(MODEL, s) && P.col[s] >= 0) SENS[((row0 + k) * P.n_id + P.col[s]) * B + b] = Fd[s];
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
// (the sums of k_id_normal, cfx_ident.h), written to the workspace WS [E][1 + n + n (n + 1) / 2][B]: row 0 the cost,
// rows 1 .. n the gradient, then the packed Gauss-Newton lower triangle, in the caller's columns.
// ---------------------------------------------------------------------------------------------------
template <int MODEL, int SCHEME, int D>
__global__ void __launch_bounds__(kIdmBlock) k_idm_normal(const IdmParams P, const double* __restrict__ theta,
                                                          double* __restrict__ WS) {
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
    idm_shoot<MODEL, SCHEME, D>(P, theta, b, e, [&](int k, double F, const double (&Fd)[D]) {
        const double w = P.weight[(int64_t)k * E + e];
        const double r = F - P.target[(int64_t)k * E + e];
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
    const double dt = P.final_time[e] / (double)P.n_shooting[e], dt2 = 2.0 * dt;
    const int n = P.n_id;
    double* ws = WS + (int64_t)e * (1 + n + n * (n + 1) / 2) * B + b;
    ws[0] = dt * cost;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (!id_has(MODEL, i) || P.col[i] < 0) continue;
        const int ci = P.col[i];
        ws[(int64_t)(1 + ci) * B] = dt2 * g[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            if (!id_has(MODEL, j) || P.col[j] < 0) continue;
            const int cj = P.col[j];
            const int hi = ci > cj ? ci : cj, lo = ci > cj ? cj : ci;
            ws[(int64_t)(1 + n + hi * (hi + 1) / 2 + lo) * B] = dt2 * H[i * (i + 1) / 2 + j];
        }
    }
}

hipError_t launch_idm_sens(int model, int scheme, int d, const IdmParams& P, const double* theta, double* force,
                           double* sens, hipStream_t s);
hipError_t launch_idm_normal(int model, int scheme, int d, const IdmParams& P, const double* theta, double* ws,
                             double* cost, double* grad, double* gn, double* cost_per_train, hipStream_t s);
// The sum over the trains of a workspace WS [E][1 + n + n (n + 1) / 2][B], in train order (also cfx_idfm.h's).
hipError_t launch_idm_reduce(int64_t B, int E, int n, const double* ws, double* cost, double* grad, double* gn,
                             double* cost_per_train, hipStream_t s);

}  // namespace cfx
