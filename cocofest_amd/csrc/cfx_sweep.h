// cfx_sweep.h — gfx950 kernel of the stimulation-train sweep (cfx_sweep_integrate, cfx_sweep_score).
//
// One thread per instance, and every instance carries its OWN train: pulse times, pulse count, truncation,
// n_shooting, final_time and per-pulse widths / intensities.  Single shooting from the rest state (or a given x0)
// over N_b intervals x m sub-steps of any of the six models, RK1 / RK2 / RK4, no tangents.  Nothing is tabulated on
// the host: the calcium forcing is formed here from the instance's pulses.
//
// Per-instance data is SoA [element][B] (lane b of a wave reads element e at e * B + b):
//     times [P][B], act [P][B] (int32), value [P][B] (Ding2007 width / Hmed2018 intensity; Ding2003: unused),
//     n_pulses, truncation, n_shooting [B] (int32), final_time [B].
// act[i] is pulse i's ACTIVATION NODE: the first node k with t_i <= k final_time / N in exact rational arithmetic,
// computed by the host (the rule of get_numerical_data_time_series).  The kernel never compares floating-point
// times: at interval k the visible pulses are those with act <= k, the window the last `truncation` of them, and it
// is constant inside the interval.
//
// Calcium forcing (ding2003.py:200-252), factorised on the interval start t_k = k dt as in cfx_ident.h:
//     cs(t) = sum_window r_i lambda_i exp(-(t - t_i) / tauc) = exp(-(t - t_k) / tauc) G_k,
//     G_k   = sum_window r_i lambda_i exp(-(t_k - t_i) / tauc),
//     r_i   = 1 for the first pulse of the window, else 1 + (r0 - 1) exp(-(t_i - t_{i-1}) / tauc),
// r0 = km_rest + r0_km (the constant, with fatigue too), lambda_i = 1 (Ding) or ar (tanh(bs (I_i - Is)) + cr) (Hmed).
// G_k is folded once per interval in a loop over the window that keeps no per-pulse register, so the truncation is
// unbounded; both exponents are <= 0 (t_i <= t_k <= t), so nothing overflows.  The stage factors of sub-step j are
// exp(-j h / tauc) (one exp), that times the constant exp(-h / (2 tauc)) for the midpoint, and the next sub-step's
// own factor for the end point.  An empty window gives cs = 0.
//
// The state is at most five doubles; the thread's only other live values are the interval's G, the Ding2007
// amplitude factor and a handful of constants.  No cross-thread arithmetic, no atomics, no LDS: an instance's result
// does not depend on its position in the batch or on its neighbours.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cfx_kernels.h"

namespace cfx {

struct SweepParams {
    int64_t B;            // instances
    int32_t P, Nmax, m;   // pulse rows, node rows - 1 of the node output, RK sub-steps per interval
    double inv_tauc, r0m1, mult, tau2;        // r0m1 = km_rest + r0_km - 1
    double a_rest, tau1_rest, km_rest;        // a_rest: a_scale for Ding2007
    double pd0, inv_pdt, ar, bs, Is, cr;
    double alpha_a, alpha_tau1, alpha_km, inv_tau_fat;
    const double* times;
    const int32_t* act;
    const double* value;
    const int32_t* n_pulses;
    const int32_t* truncation;
    const int32_t* n_shooting;
    const double* final_time;
    const double* x0;   // [nx][B] or nullptr: the rest state
    double* xf;         // [nx][B]
    double* nodes;      // [(Nmax + 1)][nx][B] or nullptr
    // k_sweep<.., SCORE = true> only (cfx_sweep_score): the target force and the metrics
    const double* ty;   // [tn] samples of the target at t = j * sample_dt
    int32_t tn;         // >= 1
    double inv_sdt;     // 1.0 / sample_dt
    double* metrics;    // [kSweepMetrics][B]
};

constexpr int kSweepMetrics = 6;  // CFX_SWEEP_N_METRICS: track, impulse, peak, peak_node, end_error, mean_force

// The target force at time t >= 0: piecewise linear through the samples, the last one held beyond the table.
__device__ __forceinline__ double sweep_target(const SweepParams& P, double t) {
    const int last = P.tn - 1;
    const double u = t * P.inv_sdt;
    if (last == 0 || !(u < (double)last)) return P.ty[last];  // floor(u) >= tn - 1
    const int j = (int)floor(u);
    const double y0 = P.ty[j];
    return fma(u - (double)j, P.ty[j + 1] - y0, y0);
}

// One right-hand side.  x = (cn, F[, A, Tau1, Km]); cs: the calcium forcing at the stage time; amp: Ding2007 E(pw).
template <int MODEL>
__device__ __forceinline__ void sweep_rhs(const SweepParams& P, double cs, double amp, const double (&x)[nx_of(MODEL)],
                                          double (&k)[nx_of(MODEL)]) {
    constexpr bool FAT = is_fatigue(MODEL);
    const double cn = x[0], F = x[1];
    double A = P.a_rest, tau1 = P.tau1_rest, km = P.km_rest;
    if constexpr (FAT) {
        A = x[2];
        tau1 = x[3];
        km = x[4];
    }
    k[0] = P.inv_tauc * (cs - cn);  // ding2003.py:254-266
    // force row in the single-reciprocal form of rhs_force (cfx_kernels.h)
    const double Aeff = is_pw(MODEL) ? A * amp : A;
    const double d1 = km + cn;
    const double d2 = fma(tau1, d1, P.tau2 * cn);
    const double R = frcp(d1 * d2);
    const double s1 = cn * (d2 * R);  // s = cn / d1
    const double t2 = d1 * (d1 * R);  // 1 / (tau1 + tau2 s) = d1 / d2
    k[1] = P.mult * (Aeff * s1 - F * t2);
    if constexpr (FAT) {
        k[2] = P.alpha_a * F - (A - P.a_rest) * P.inv_tau_fat;
        k[3] = P.alpha_tau1 * F - (tau1 - P.tau1_rest) * P.inv_tau_fat;
        k[4] = P.alpha_km * F - (km - P.km_rest) * P.inv_tau_fat;
    }
}

// One wave per block: instances do different amounts of work (N_b m steps x window length), so small blocks spread
// a sorted batch over more compute units and a block's registers are freed as soon as its own wave is done.
constexpr int kSweepBlock = 64;

// SCORE (cfx_sweep_score): the same rollout, with the functionals of the node forces F_0..F_N against the target
// carried in registers: sum_k (F_k - y(t_k))^2, the trapezoid sum, the peak and its first node.  The target is read
// at the node times only (N + 1 lookups), the sums run sequentially in k, and the six metrics are written once at
// the end; no node is written.  SCORE = false compiles to the code it was before the parameter existed.
template <int MODEL, int SCHEME, bool SCORE = false>
__global__ void __launch_bounds__(kSweepBlock) k_sweep(const SweepParams P) {
    constexpr int NX = nx_of(MODEL);
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int np = P.n_pulses[b], T = P.truncation[b], N = P.n_shooting[b];
    const double dt = P.final_time[b] / (double)N;
    const double h = dt / (double)P.m, h2 = 0.5 * h, h6 = h / 6.0;
    const double eh2 = exp(-h2 * P.inv_tauc);

    double x[NX];
    x[0] = x[1] = 0.0;
    if constexpr (NX == 5) {
        x[2] = P.a_rest;
        x[3] = P.tau1_rest;
        x[4] = P.km_rest;
    }
    if (P.x0 != nullptr) {
#pragma unroll
        for (int r = 0; r < NX; ++r) x[r] = P.x0[(int64_t)r * B + b];
    }
    if (P.nodes != nullptr) {
#pragma unroll
        for (int r = 0; r < NX; ++r) P.nodes[(int64_t)r * B + b] = x[r];
    }
    // SCORE: node 0 counts, with F_0 from x0
    double trk = 0.0, trap = 0.0, peak = 0.0, err = 0.0;
    int peak_node = 0;
    if constexpr (SCORE) {
        err = x[1] - sweep_target(P, 0.0);
        trk = err * err;
        trap = 0.5 * x[1];
        peak = x[1];
    }

    int nv = 0;  // visible pulses
    for (int k = 0; k < N; ++k) {
        while (nv < np && P.act[(int64_t)nv * B + b] <= k) ++nv;
        const int lo = nv > T ? nv - T : 0;
        const double tk = (double)k * dt;
        double G = 0.0, tprev = 0.0;
        for (int i = lo; i < nv; ++i) {
            const double ti = P.times[(int64_t)i * B + b];
            double w = i == lo ? 1.0 : fma(P.r0m1, exp(-(ti - tprev) * P.inv_tauc), 1.0);
            if constexpr (is_int(MODEL))  // hmed2018.py:169-180
                w *= P.ar * (tanh(P.bs * (P.value[(int64_t)i * B + b] - P.Is)) + P.cr);
            G = fma(w, exp(-(tk - ti) * P.inv_tauc), G);
            tprev = ti;
        }
        double amp = 1.0;
        if constexpr (is_pw(MODEL)) {
            // ding2007.py:172-188, the width of the last visible pulse (the first one's before any is visible)
            if (np > 0) {
                const double pw = P.value[(int64_t)(nv > 0 ? nv - 1 : 0) * B + b];
                amp = 1.0 - exp(-(pw - P.pd0) * P.inv_pdt);
            }
        }
        double ea = 1.0;  // exp(-(t - t_k) / tauc) at the start of the sub-step
        for (int j = 0; j < P.m; ++j) {
            double k1[NX];
            sweep_rhs<MODEL>(P, ea * G, amp, x, k1);
            const double eb = exp(-((double)(j + 1) * h) * P.inv_tauc);
            if constexpr (SCHEME == 1) {
#pragma unroll
                for (int r = 0; r < NX; ++r) x[r] = x[r] + h * k1[r];
            } else if constexpr (SCHEME == 2) {
                double xs[NX], k2[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) xs[r] = x[r] + h2 * k1[r];
                sweep_rhs<MODEL>(P, (ea * eh2) * G, amp, xs, k2);
#pragma unroll
                for (int r = 0; r < NX; ++r) x[r] = x[r] + h * k2[r];
            } else {
                const double cm = (ea * eh2) * G;
                double xs[NX], kk[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) xs[r] = x[r] + h2 * k1[r];
#pragma unroll
                for (int sg = 1; sg < 4; ++sg) {
                    sweep_rhs<MODEL>(P, sg < 3 ? cm : eb * G, amp, xs, kk);
                    if (sg < 3) {
                        const double c = sg == 1 ? h2 : h;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            k1[r] = k1[r] + 2.0 * kk[r];  // k1 accumulates k1 + 2 k2 + 2 k3
                            xs[r] = x[r] + c * kk[r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) x[r] = x[r] + h6 * (k1[r] + kk[r]);
            }
            ea = eb;
        }
        if (P.nodes != nullptr) {
#pragma unroll
            for (int r = 0; r < NX; ++r) P.nodes[((int64_t)(k + 1) * NX + r) * B + b] = x[r];
        }
        if constexpr (SCORE) {
            const double F = x[1];
            err = F - sweep_target(P, (double)(k + 1) * dt);
            trk = fma(err, err, trk);
            trap += k + 1 < N ? F : 0.5 * F;
            if (F > peak) {
                peak = F;
                peak_node = k + 1;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < NX; ++r) P.xf[(int64_t)r * B + b] = x[r];
    if constexpr (SCORE) {
        const double impulse = dt * trap;
        P.metrics[b] = dt * trk;
        P.metrics[B + b] = impulse;
        P.metrics[2 * B + b] = peak;
        P.metrics[3 * B + b] = (double)peak_node;
        P.metrics[4 * B + b] = err;  // of the last node
        P.metrics[5 * B + b] = impulse / P.final_time[b];
    }
    if (P.nodes != nullptr) {
        const double nan = __builtin_nan("");
        for (int k = N + 1; k <= P.Nmax; ++k) {
#pragma unroll
            for (int r = 0; r < NX; ++r) P.nodes[((int64_t)k * NX + r) * B + b] = nan;
        }
    }
}

hipError_t launch_sweep(int model, int scheme, const SweepParams& P, hipStream_t s);
hipError_t launch_sweep_score(int model, int scheme, const SweepParams& P, hipStream_t s);  // k_sweep<.., true>

}  // namespace cfx
