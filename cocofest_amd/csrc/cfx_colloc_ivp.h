// cfx_colloc_ivp.h — implicit collocation integrator (cfx_integrate on a collocation handle; IvpFes with
// OdeSolver.COLLOCATION, cocofest/integration/ivp_fes.py:223-227).
//
// Thread = one instance, sequential over the N intervals (as k_ivp).  In interval k the d nx unknowns
// x_k^1..x_k^d solve the defect rows of cfx_colloc.h,
//   sum_i C[i][j] x_k^i - dt f(t_k + tau_j dt, x_k^j, u_k) = 0,  j = 1..d,  x_k^0 given,
// and the next node state is sum_i D[i] x_k^i, accumulated in k_colloc's operation order so that the continuity
// rows of eval_g vanish exactly at the trajectory.  With Chat[j][i] = C[i][j] (i, j >= 1) and c0[j] = C[0][j] the
// structure of the right-hand sides (rhs_force, cfx_kernels.h) reduces the d nx system to d unknowns:
//   calcium   (cs_j - Cn) / tauc is linear in Cn alone:  (Chat + (dt / tauc) I) Cn = (dt / tauc) cs - c0 Cn^0.
//             The matrix is the same for every interval and instance; the host inverts it once (civp_tables):
//             Cn^j = vc0[j] Cn^0 + sum_i McS[j][i] cs_i.
//   fatigue   A, Tau1, Km: y' = alpha F - (y - y_rest) / tau_fat, linear in y and F with the constant matrix
//             Chat + (dt / tau_fat) I:  y^j = vf0[j] y^0 + wf[j] y_rest + alpha Gd_j,  Gd = (dt Mf) F  (one product
//             serves the three states).
//   force     without fatigue linear in F once Cn is known:  (Chat + diag(-dt df/dF)) F = dt f(F = 0) - c0 F^0, one
//             d x d solve, no iteration.  With fatigue a Newton iteration on F^1..F^d alone, whose matrix is
//             Chat - dt (df/dF I + (df/dA alpha_A + df/dTau1 alpha_Tau1 + df/dKm alpha_Km) dt Mf).
// The d x d solves use Gaussian elimination with partial pivoting.  Degrees 1..5 are compile-time: the system lives
// in registers, the loops are unrolled and a row exchange is a select over the candidate rows (no dynamic register
// indexing, hence no scratch).  Degrees 6..9 run the same body with the system in LDS, element-major and
// lane-minor (conflict-free), 117 doubles per lane.
//
// Newton termination (fatigue models): after applying the update delta the iteration stops when
//   max_j |delta_j| <= 2^-40 max_j |F^j|.
// Newton converges quadratically here (the only nonlinearity in F is the fatigue coupling, alpha ~ 1e-5 and below),
// so an update of relative size eta leaves an error O(eta^2) < 2^-80: the accepted iterate is at rounding level.  A
// threshold nearer the unit roundoff could be missed on the rounding noise of the solve alone (cond(J) eps, cond up
// to ~1e3 at d = 9) and reach the cap on a converged iterate.  At most kCivpMaxIter = 20 updates: an interval that
// has not met the test by then marks the instance failed; its points and every later sample are written as NaN and
// the status is -(k + 1).  A NaN anywhere in the update fails the test, so it ends the same way.  The linear
// solves report 0 iterations; a non-finite result (singular matrix) fails the interval likewise.
//
// Trajectory: for each interval x_k^0, x_k^1..x_k^d, then x_N: traj[(s nx + r) B + b], s = k (d + 1) + j.
#pragma once

#include "cfx_kernels.h"

namespace cfx {

constexpr int kCivpMaxIter = 20;
constexpr int kCivpBlock = 64;                      // lanes per workgroup (one wave)
constexpr int kCivpLds = kMaxDeg * kMaxDeg + 4 * kMaxDeg;  // generic body: J, rhs / delta, F, Cn, Gd per lane

// offsets (in doubles) of the host-built tables of degree d: McS [d d], vc0 [d], MfD [d d], vf0 [d], wf [d]
constexpr int civp_off_vc0(int d) { return d * d; }
constexpr int civp_off_mf(int d) { return d * d + d; }
constexpr int civp_off_vf0(int d) { return 2 * d * d + d; }
constexpr int civp_off_wf(int d) { return 2 * d * d + 2 * d; }
constexpr int civp_table_len(int d) { return 2 * d * d + 3 * d; }

// Solve A x = b in place (x in b) by Gaussian elimination with partial pivoting.  A(r, c), b(r): accessors.
// DEG > 0: every loop unrolls and the row exchange is a select over the rows below the pivot.
template <int DEG, class MA, class VB>
CFX_HD void civp_solve(int d, MA&& A, VB&& b) {
    constexpr int UN = DEG > 0 ? DEG : 1;
#pragma unroll UN
    for (int c = 0; c < d; ++c) {
        int p = c;
        double best = fabs(A(c, c));
#pragma unroll UN
        for (int r = c + 1; r < d; ++r) {
            const double a = fabs(A(r, c));
            if (a > best) {
                best = a;
                p = r;
            }
        }
        if constexpr (DEG > 0) {
#pragma unroll UN
            for (int r = c + 1; r < d; ++r) {
                const bool sw = p == r;
#pragma unroll UN
                for (int cc = c; cc < d; ++cc) {
                    const double t = A(c, cc), s = A(r, cc);
                    A(c, cc) = sw ? s : t;
                    A(r, cc) = sw ? t : s;
                }
                const double t = b(c), s = b(r);
                b(c) = sw ? s : t;
                b(r) = sw ? t : s;
            }
        } else if (p != c) {
            for (int cc = c; cc < d; ++cc) {
                const double t = A(c, cc);
                A(c, cc) = A(p, cc);
                A(p, cc) = t;
            }
            const double t = b(c);
            b(c) = b(p);
            b(p) = t;
        }
        const double inv = 1.0 / A(c, c);
        A(c, c) = inv;
#pragma unroll UN
        for (int r = c + 1; r < d; ++r) {
            const double m = A(r, c) * inv;
#pragma unroll UN
            for (int cc = c + 1; cc < d; ++cc) A(r, cc) = fma(-m, A(c, cc), A(r, cc));
            b(r) = fma(-m, b(c), b(r));
        }
    }
#pragma unroll UN
    for (int c = d - 1; c >= 0; --c) {
        double s = b(c);
#pragma unroll UN
        for (int cc = c + 1; cc < d; ++cc) s = fma(-A(c, cc), b(cc), s);
        b(c) = s * A(c, c);
    }
}

// DEG > 0: compile-time degree, register-resident system.  DEG == 0: any degree up to kMaxDeg, system in LDS.
template <int MODEL, int TMAX, int DEG>
__global__ void __launch_bounds__(kCivpBlock) k_colloc_ivp(const KParams P, const double* __restrict__ TB,
                                                           const double* __restrict__ X0,
                                                           const double* __restrict__ U, double* __restrict__ TR,
                                                           int32_t* __restrict__ ST) {
    constexpr int NX = nx_of(MODEL);
    constexpr bool FAT = is_fatigue(MODEL), PW = is_pw(MODEL), HM = is_int(MODEL);
    constexpr int DM = DEG > 0 ? DEG : 1;
    constexpr int UN = DEG > 0 ? DEG + 1 : 1;
    constexpr int NUR = PW ? 1 : (HM ? TMAX : 1);  // controls held in registers
    __shared__ double ws[DEG > 0 ? 1 : kCivpLds * kCivpBlock];
    const int64_t B = P.B;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int d = DEG > 0 ? DEG : P.deg;
    const int tid = threadIdx.x;
    (void)tid;

    // the interval's system: registers (DEG > 0) or LDS, element e of this lane at ws[e * kCivpBlock + tid]
    double Jr[DM][DM], Rr[DM], Fr[DM], Cr[DM], Gr[DM];
    auto Jm = [&](int r, int c) -> double& {
        if constexpr (DEG > 0) return Jr[r][c];
        else return ws[(r * kMaxDeg + c) * kCivpBlock + tid];
    };
    auto Rv = [&](int j) -> double& {
        if constexpr (DEG > 0) return Rr[j];
        else return ws[(kMaxDeg * kMaxDeg + j) * kCivpBlock + tid];
    };
    auto Fv = [&](int j) -> double& {
        if constexpr (DEG > 0) return Fr[j];
        else return ws[(kMaxDeg * kMaxDeg + kMaxDeg + j) * kCivpBlock + tid];
    };
    auto Cv = [&](int j) -> double& {
        if constexpr (DEG > 0) return Cr[j];
        else return ws[(kMaxDeg * kMaxDeg + 2 * kMaxDeg + j) * kCivpBlock + tid];
    };
    auto Gv = [&](int j) -> double& {
        if constexpr (DEG > 0) return Gr[j];
        else return ws[(kMaxDeg * kMaxDeg + 3 * kMaxDeg + j) * kCivpBlock + tid];
    };
    const double* McS = TB;
    const double* vc0 = TB + civp_off_vc0(d);
    const double* MfD = TB + civp_off_mf(d);
    const double* vf0 = TB + civp_off_vf0(d);
    const double* wf = TB + civp_off_wf(d);
    const double restv[5] = {0.0, 0.0, P.a_fat_rest, P.tau1_rest, P.km_rest};
    const double alph[5] = {0.0, 0.0, P.alpha_a, P.alpha_tau1, P.alpha_km};
    const double qnan = __builtin_nan("");

    double x0[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        x0[r] = X0 ? X0[(int64_t)r * B + b] : P.rest[r];
        TR[(int64_t)r * B + b] = x0[r];
    }
    // controls of interval 0; those of interval k + 1 are loaded before interval k's stores (on CDNA a load issued
    // after stores waits for them)
    double un[NUR];
    auto load_u = [&](int k) {
#pragma unroll
        for (int i = 0; i < NUR; ++i) {
            un[i] = HM ? P.Is : 0.0;
            if ((PW || HM) && i < P.nu && k < P.N) un[i] = U[((int64_t)k * P.nu + i) * B + b];
        }
    };
    load_u(0);

    int maxit = 0, kfail = -1;
    for (int k = 0; k < P.N; ++k) {
        const int64_t s0 = (int64_t)k * (d + 1);
        if (kfail >= 0) {  // a failed instance: NaN to the end
            for (int j = 1; j <= d + 1; ++j)
#pragma unroll
                for (int r = 0; r < NX; ++r) TR[((s0 + j) * NX + r) * B + b] = qnan;
            continue;
        }
        Amp amp{1.0, 0.0, -1};
        if constexpr (PW) {
            const double ex = exp(-(un[0] - P.pd0) / P.pdt);
            amp.E = 1.0 - ex;
            amp.dE = ex / P.pdt;
        }
        double lam[HM ? TMAX : 1];
        if constexpr (HM) {
#pragma unroll
            for (int i = 0; i < TMAX; ++i) lam[i] = i < P.T ? P.ar * (tanh(P.bs * (un[i] - P.Is)) + P.cr) : 0.0;
        }
        // calcium: the stimulation sums of the d points (into R), then Cn = vc0 Cn^0 + McS cs
#pragma unroll UN
        for (int j = 0; j < d; ++j) {
            const double* coef = P.tab + (int64_t)(k * d + j) * (HM ? TMAX : 1);
            double cs;
            if constexpr (HM) {
                cs = 0.0;
#pragma unroll
                for (int i = 0; i < TMAX; ++i) cs += coef[i] * lam[i];
            } else {
                cs = coef[0];
            }
            Rv(j) = cs;
        }
#pragma unroll UN
        for (int j = 0; j < d; ++j) {
            double cn = vc0[j] * x0[0];
#pragma unroll UN
            for (int i = 0; i < d; ++i) cn = fma(McS[j * d + i], Rv(i), cn);
            Cv(j) = cn;
        }
        // force: F^j starts at F^0; one pass without fatigue (the system is linear and solved for F itself)
#pragma unroll UN
        for (int j = 0; j < d; ++j) Fv(j) = FAT ? x0[1] : 0.0;
        bool ok = false;
        int it = 0;
        for (; it < (FAT ? kCivpMaxIter : 1) && !ok; ++it) {
            if constexpr (FAT) {
#pragma unroll UN
                for (int j = 0; j < d; ++j) {
                    double g = 0.0;
#pragma unroll UN
                    for (int i = 0; i < d; ++i) g = fma(MfD[j * d + i], Fv(i), g);
                    Gv(j) = g;
                }
            }
#pragma unroll UN
            for (int j = 0; j < d; ++j) {
                double x[NX], f[NX], fd[NX][NX], xd[NX][NX], cnd[NX];
                x[0] = Cv(j);
                x[1] = Fv(j);
                if constexpr (FAT) {
#pragma unroll
                    for (int r = 2; r < NX; ++r) x[r] = fma(alph[r], Gv(j), fma(vf0[j], x0[r], wf[j] * restv[r]));
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    cnd[r] = r == 0 ? 1.0 : 0.0;
#pragma unroll
                    for (int c = 0; c < NX; ++c) xd[r][c] = r == c ? 1.0 : 0.0;
                }
                rhs_force<MODEL, NX, true>(P, x[0], cnd, x, xd, amp, f, fd);
                double coup = 0.0;
                if constexpr (FAT) coup = fd[1][2] * alph[2] + fd[1][3] * alph[3] + fd[1][4] * alph[4];
                // fatigue: R = -(defect row) at the iterate; otherwise the right-hand side dt f(F = 0) - c0 F^0
                double poly = P.colC[0][j + 1] * x0[1];
#pragma unroll UN
                for (int i = 0; i < d; ++i) {
                    if (FAT) poly = fma(P.colC[i + 1][j + 1], Fv(i), poly);
                    double a = P.colC[i + 1][j + 1];
                    if (i == j) a = fma(-P.dt, fd[1][1], a);
                    if (FAT) a = fma(-P.dt * coup, MfD[j * d + i], a);
                    Jm(j, i) = a;
                }
                Rv(j) = fma(P.dt, f[1], -poly);
            }
            civp_solve<DEG>(d, Jm, Rv);
            if constexpr (FAT) {
                double dmax = 0.0, fnorm = 0.0;
                bool fin = true;
#pragma unroll UN
                for (int j = 0; j < d; ++j) {
                    const double dl = Rv(j);
                    Fv(j) += dl;
                    fin = fin && (fabs(dl) <= 1.7976931348623157e308);
                    dmax = fmax(dmax, fabs(dl));
                    fnorm = fmax(fnorm, fabs(Fv(j)));
                }
                ok = fin && dmax <= 0x1p-40 * fnorm;
            } else {
                bool fin = true;
#pragma unroll UN
                for (int j = 0; j < d; ++j) {
                    Fv(j) = Rv(j);
                    fin = fin && (fabs(Rv(j)) <= 1.7976931348623157e308);
                }
                ok = fin;
            }
        }
        if (FAT) {
            maxit = it > maxit ? it : maxit;
            if (ok) {  // the fatigue states of the accepted iterate
#pragma unroll UN
                for (int j = 0; j < d; ++j) {
                    double g = 0.0;
#pragma unroll UN
                    for (int i = 0; i < d; ++i) g = fma(MfD[j * d + i], Fv(i), g);
                    Gv(j) = g;
                }
            }
        }
        if (!ok) kfail = k;
        // the next interval's controls, ahead of this interval's stores
        load_u(k + 1);
        double xn[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) xn[r] = fma(P.colD[0], x0[r], 0.0);
#pragma unroll UN
        for (int j = 0; j < d; ++j) {
            double x[NX];
            x[0] = Cv(j);
            x[1] = Fv(j);
            if constexpr (FAT) {
#pragma unroll
                for (int r = 2; r < NX; ++r) x[r] = fma(alph[r], Gv(j), fma(vf0[j], x0[r], wf[j] * restv[r]));
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                xn[r] = fma(P.colD[j + 1], x[r], xn[r]);
                TR[((s0 + j + 1) * NX + r) * B + b] = ok ? x[r] : qnan;
            }
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            x0[r] = xn[r];
            TR[((s0 + d + 1) * NX + r) * B + b] = ok ? xn[r] : qnan;
        }
    }
    ST[b] = kfail >= 0 ? -(kfail + 1) : maxit;
}

}  // namespace cfx
