// cfx_api_trains.hip — the C ABI of the three stimulation-train families of libcfx (include/cfx.h): cfx_sweep_*,
// cfx_idm_* and cfx_idfm_*.  Their handles are one session core (device, stream, staging buffers, error string) plus
// the kernel parameters of the family; the kernels are cfx_sweep.h, cfx_idm.h and cfx_idfm.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/cfx.h"
#include "cfx_idfm.h"
#include "cfx_idm.h"
#include "cfx_internal.h"
#include "cfx_sweep.h"

using namespace cfx;

// ------------------------------------------------------------------------------------------------------
// the session core of every train family
// ------------------------------------------------------------------------------------------------------
namespace {

struct TrainSession {
    int model = 0, scheme = 1, device = 0;
    // E: the minor extent of the train arrays (the trains of an identification; a sweep has one per instance, E = B)
    int64_t B = 0, E = 0;
    int32_t P = 0, Nmax = 0, m = 1;
    bool needs_value = false;
    hipStream_t stream = nullptr;
    // staging of host calls: times, value, final_time, then the family's own arrays (doubles); act [P][E] + the three
    // counts [E] (int32)
    DevBuf dbuf[9];
    int32_t* d_int = nullptr;
    double* d_ws = nullptr;  // identification: the per-train normal equations (host and device calls)
    std::string err;
};

static int session_fail(TrainSession* s, int code, const std::string& msg) {
    s->err = msg;
    return code;
}

static const char* session_error(const TrainSession* s) { return s ? s->err.c_str() : g_create_error.c_str(); }

#define TRAIN_HIP(call)                                                                                            \
    do {                                                                                                           \
        hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess) return session_fail(s, CFX_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class H>
static void session_close(H* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (DevBuf& b : s->dbuf)
        if (b.p) (void)hipFree(b.p);
    if (s->d_int) (void)hipFree(s->d_int);
    if (s->d_ws) (void)hipFree(s->d_ws);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// What every create function does after its own argument checks: the device, the handle with its core filled, the
// stream and (ws > 0) a workspace of ws doubles.
template <class H>
static int session_open(const char* fn, int model, int scheme, int n_steps, int64_t B, int64_t E, int32_t P,
                        int32_t Nmax, int device, size_t ws, H** out) {
    const std::string f = std::string(fn) + ": ";
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return g_create_error = f + "no HIP device available (libcfx has no CPU path)", CFX_ENODEV;
    if (device < 0 || device >= ndev) return g_create_error = f + "bad device ordinal", CFX_ENODEV;
    H* s = new H();
    s->model = model;
    s->scheme = scheme;
    s->device = device;
    s->B = B;
    s->E = E;
    s->P = P;
    s->Nmax = Nmax;
    s->m = n_steps;
    s->needs_value = is_pw(model) || is_int(model);
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        s->stream = nullptr;
        session_close(s);
        return g_create_error = f + "could not create a stream on the device", CFX_EHIP;
    }
    if (ws && hipMalloc((void**)&s->d_ws, ws * sizeof(double)) != hipSuccess) {
        s->d_ws = nullptr;
        session_close(s);
        return g_create_error = f + "hipMalloc of the workspace failed", CFX_ENOMEM;
    }
    *out = s;
    return CFX_OK;
}

// device buffer `slot` of at least n doubles
static double* session_buf(TrainSession* s, const char* fn, int slot, size_t n, int* rc) {
    DevBuf& b = s->dbuf[slot];
    if (b.n < n) {
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr;
        b.n = 0;
        if (hipMalloc(&b.p, n * sizeof(double)) != hipSuccess) {
            b.p = nullptr;
            *rc = session_fail(s, CFX_ENOMEM, std::string(fn) + ": hipMalloc failed");
            return nullptr;
        }
        b.n = n;
    }
    return b.p;
}

// The model constants that the kernels of the sweep and of the fatigue identification read under the same names.
template <class Params>
static void fill_model_constants(int model, const cfx_constants* c, Params& p) {
    p.inv_tauc = 1.0 / c->tauc;
    p.r0m1 = c->km_rest + c->r0_km_relationship - 1.0;
    p.mult = c->fl * c->fv + c->fp;
    p.tau2 = c->tau2;
    p.a_rest = is_pw(model) ? c->a_scale : c->a_rest;  // ding2007_with_fatigue.py:198-241: A relaxes to a_scale
    p.tau1_rest = c->tau1_rest;
    p.km_rest = c->km_rest;
    p.pd0 = c->pd0;
    p.inv_pdt = is_pw(model) ? 1.0 / c->pdt : 0.0;
    p.ar = c->ar;
    p.bs = c->bs;
    p.Is = c->Is;
    p.cr = c->cr;
}

// The seven train arrays of a cfx_sweep_trains or a cfx_idm_trains ([..][E], the same names in both), and the two
// ways of handing them to a kernel's parameters (SweepParams, IdmParams or IdfmParams: the same seven names).
struct TrainView {
    bool given;  // false: no arrays (a check of the creation arguments alone)
    const double* times;
    const int32_t* act_node;
    const double* value;
    const int32_t *n_pulses, *truncation, *n_shooting;
    const double* final_time;

    bool has_null(bool needs_value) const {
        return !times || !act_node || !n_pulses || !truncation || !n_shooting || !final_time || (needs_value && !value);
    }

    // CFX_DEVICE: the caller's own device arrays
    template <class Params>
    void point(Params& p) const {
        p.times = times;
        p.act = act_node;
        p.value = value;
        p.n_pulses = n_pulses;
        p.truncation = truncation;
        p.n_shooting = n_shooting;
        p.final_time = final_time;
    }

    // Host arrays: their upload into the session's buffers on its stream.  between(): the family's own uploads, which
    // go after the double arrays and before the int32 block (a CFX_* code).
    template <class Params, class Between>
    int upload(TrainSession* s, const char* fn, Params& p, Between&& between) const {
        const size_t E = (size_t)s->E, P = (size_t)s->P;
        int rc = CFX_OK;
        double* d_t = session_buf(s, fn, 0, P * E, &rc);
        double* d_v = s->needs_value ? session_buf(s, fn, 1, P * E, &rc) : nullptr;
        double* d_tf = session_buf(s, fn, 2, E, &rc);
        if (!d_t || (s->needs_value && !d_v) || !d_tf) return rc;
        if (!s->d_int && hipMalloc(&s->d_int, (P + 3) * E * sizeof(int32_t)) != hipSuccess) {
            s->d_int = nullptr;
            return session_fail(s, CFX_ENOMEM, std::string(fn) + ": hipMalloc failed");
        }
        int32_t* d_cnt = s->d_int + P * E;
        hipStream_t q = s->stream;
        TRAIN_HIP(hipMemcpyAsync(d_t, times, P * E * sizeof(double), hipMemcpyHostToDevice, q));
        if (d_v) TRAIN_HIP(hipMemcpyAsync(d_v, value, P * E * sizeof(double), hipMemcpyHostToDevice, q));
        TRAIN_HIP(hipMemcpyAsync(d_tf, final_time, E * sizeof(double), hipMemcpyHostToDevice, q));
        if ((rc = between()) != CFX_OK) return rc;
        TRAIN_HIP(hipMemcpyAsync(s->d_int, act_node, P * E * sizeof(int32_t), hipMemcpyHostToDevice, q));
        TRAIN_HIP(hipMemcpyAsync(d_cnt, n_pulses, E * sizeof(int32_t), hipMemcpyHostToDevice, q));
        TRAIN_HIP(hipMemcpyAsync(d_cnt + E, truncation, E * sizeof(int32_t), hipMemcpyHostToDevice, q));
        TRAIN_HIP(hipMemcpyAsync(d_cnt + 2 * E, n_shooting, E * sizeof(int32_t), hipMemcpyHostToDevice, q));
        TrainView{true, d_t, s->d_int, d_v, d_cnt, d_cnt + E, d_cnt + 2 * E, d_tf}.point(p);
        return CFX_OK;
    }
};

template <class Trains>
static TrainView train_view(const Trains* t) {
    if (!t) return TrainView{};
    return TrainView{true, t->times, t->act_node, t->value, t->n_pulses, t->truncation, t->n_shooting, t->final_time};
}

// The creation arguments of every family (E: the train count, a sweep's batch) and (tr.given) the host arrays of the
// trains.  unit: what carries a train in the messages, "instance" or "train".
static int train_check(const char* fn, int model, int scheme, int n_steps, int64_t E, int P, int Nmax, const char* unit,
                       const TrainView& tr, std::string& msg) {
    const std::string f = std::string(fn) + ": ";
    if (model < CFX_DING2003 || model > CFX_HMED2018_FATIGUE) return msg = f + "unknown model", CFX_EINVAL;
    if (scheme != CFX_RK1 && scheme != CFX_RK2 && scheme != CFX_RK4)
        return msg = f + "unknown scheme (must be CFX_RK1, CFX_RK2 or CFX_RK4)", CFX_EINVAL;
    if (n_steps < 1 || E < 1 || P < 1 || Nmax < 1)
        return msg = f + "n_steps, batch, max_pulses and max_shooting must be positive", CFX_EINVAL;
    if (Nmax > kMaxGridY) return msg = f + "max_shooting must be <= 65535", CFX_EINVAL;
    if (!tr.given) return CFX_OK;
    const bool needs_value = is_pw(model) || is_int(model);
    if (tr.has_null(needs_value)) return msg = f + "a train array is NULL", CFX_EINVAL;
    for (int64_t b = 0; b < E; ++b) {
        const std::string at = f + unit + " " + std::to_string(b) + ": ";
        const int N = tr.n_shooting[b], np = tr.n_pulses[b];
        if (N > kMaxGridY) return msg = at + "n_shooting must be <= 65535", CFX_EINVAL;
        if (N < 1 || N > Nmax) return msg = at + "n_shooting must be in [1, max_shooting]", CFX_EINVAL;
        if (tr.truncation[b] < 1) return msg = at + "truncation must be >= 1", CFX_EINVAL;
        if (np < 0 || np > P) return msg = at + "n_pulses must be in [0, max_pulses]", CFX_EINVAL;
        if (!(tr.final_time[b] > 0.0) || !std::isfinite(tr.final_time[b]))
            return msg = at + "final_time must be positive and finite", CFX_EINVAL;
        for (int i = 0; i < np; ++i) {
            const std::string pi = at + "pulse " + std::to_string(i) + ": ";
            const double t = tr.times[(int64_t)i * E + b];
            const int a = tr.act_node[(int64_t)i * E + b];
            if (!std::isfinite(t)) return msg = pi + "time is not finite", CFX_EINVAL;
            if (i > 0 && t < tr.times[(int64_t)(i - 1) * E + b]) return msg = pi + "time decreases", CFX_EINVAL;
            if (a < 0) return msg = pi + "activation node is negative", CFX_EINVAL;
            if (a > N) return msg = pi + "activation node past n_shooting", CFX_EINVAL;
            if (i > 0 && a < tr.act_node[(int64_t)(i - 1) * E + b])
                return msg = pi + "activation node decreases", CFX_EINVAL;
            if (needs_value && !std::isfinite(tr.value[(int64_t)i * E + b]))
                return msg = pi + "value is not finite", CFX_EINVAL;
        }
    }
    return CFX_OK;
}

}  // namespace

// the handles: the core plus the kernel parameters of the family
struct cfx_sweep : TrainSession {
    int nx = 2;
    SweepParams sp{};
};

struct cfx_idm : TrainSession {
    IdmParams ip{};
};

struct cfx_idfm : TrainSession {
    IdfmParams fp{};
};

// ------------------------------------------------------------------------------------------------------
// stimulation-train sweeps (cfx_sweep.h): every instance carries its own train
// ------------------------------------------------------------------------------------------------------
static_assert(kSweepMetrics == CFX_SWEEP_N_METRICS, "metric rows of k_sweep and of cfx.h differ");

extern "C" int cfx_sweep_check(int32_t model, int32_t scheme, int32_t n_steps, int64_t batch, int32_t max_pulses,
                               int32_t max_shooting, const cfx_sweep_trains* trains) {
    return train_check("cfx_sweep_check", model, scheme, n_steps, batch, max_pulses, max_shooting, "instance",
                       train_view(trains), g_create_error);
}

extern "C" void cfx_sweep_destroy(cfx_sweep* s) { session_close(s); }

extern "C" const char* cfx_sweep_last_error(const cfx_sweep* s) { return session_error(s); }

extern "C" int cfx_sweep_create(int32_t model, const cfx_constants* c, int32_t scheme, int32_t n_steps, int64_t batch,
                                int32_t max_pulses, int32_t max_shooting, int32_t device, cfx_sweep** out) {
    if (!c || !out) return g_create_error = "cfx_sweep_create: NULL argument", CFX_EINVAL;
    *out = nullptr;
    int rc = train_check("cfx_sweep_create", model, scheme, n_steps, batch, max_pulses, max_shooting, "instance",
                         TrainView{}, g_create_error);
    if (rc != CFX_OK) return rc;
    if (!(c->tauc > 0.0)) return g_create_error = "cfx_sweep_create: tauc must be positive", CFX_EINVAL;
    rc = session_open("cfx_sweep_create", model, scheme, n_steps, batch, batch, max_pulses, max_shooting, device, 0,
                      out);
    if (rc != CFX_OK) return rc;
    cfx_sweep* s = *out;
    s->nx = is_fatigue(model) ? 5 : 2;
    SweepParams& sp = s->sp;
    sp.B = batch;
    sp.P = max_pulses;
    sp.Nmax = max_shooting;
    sp.m = n_steps;
    fill_model_constants(model, c, sp);
    sp.alpha_a = c->alpha_a;
    sp.alpha_tau1 = c->alpha_tau1;
    sp.alpha_km = c->alpha_km;
    sp.inv_tau_fat = is_fatigue(model) ? 1.0 / c->tau_fat : 0.0;
    return CFX_OK;
}

// The checks of a target force; host: the samples too (a device caller is responsible for them).
static int sweep_target_check(const char* fn, const cfx_sweep_target* tg, bool host, std::string& msg) {
    const std::string f = std::string(fn) + ": ";
    if (!tg) return msg = f + "target is NULL", CFX_EINVAL;
    if (tg->n_samples < 1) return msg = f + "target: n_samples must be >= 1", CFX_EINVAL;
    if (tg->n_samples > 1 && !(tg->sample_dt > 0.0)) return msg = f + "target: sample_dt must be positive", CFX_EINVAL;
    if (!tg->y) return msg = f + "target: y is NULL", CFX_EINVAL;
    if (host)
        for (int32_t j = 0; j < tg->n_samples; ++j)
            if (!std::isfinite(tg->y[j]))
                return msg = f + "target: y[" + std::to_string(j) + "] is not finite", CFX_EINVAL;
    return CFX_OK;
}

extern "C" int cfx_sweep_target_check(const cfx_sweep_target* target) {
    return sweep_target_check("cfx_sweep_target_check", target, true, g_create_error);
}

// cfx_sweep_integrate (tg == nullptr) and cfx_sweep_score (tg, metrics; no nodes): one staging path, one launch.
static int sweep_run(const char* fn, cfx_sweep* s, const cfx_sweep_trains* trains, const cfx_sweep_target* tg,
                     const double* x0, double* final_state, double* nodes, double* metrics, uint32_t flags,
                     void* hip_stream) {
    const std::string f = std::string(fn) + ": ";
    const TrainView tr = train_view(trains);
    if (tr.has_null(s->needs_value)) return session_fail(s, CFX_EINVAL, f + "a train array is NULL");
    const size_t B = (size_t)s->B, nx = (size_t)s->nx, nn = (size_t)s->Nmax + 1;
    const size_t nt = tg ? (size_t)tg->n_samples : 0;
    SweepParams sp = s->sp;
    if (tg) {
        sp.tn = tg->n_samples;
        sp.inv_sdt = tg->n_samples > 1 ? 1.0 / tg->sample_dt : 1.0;
    }
    const auto launch = [&](hipStream_t st) {
        return tg ? launch_sweep_score(s->model, s->scheme, sp, st) : launch_sweep(s->model, s->scheme, sp, st);
    };
    if (hipSetDevice(s->device) != hipSuccess) return session_fail(s, CFX_EHIP, f + "hipSetDevice failed");
    if (flags & CFX_DEVICE) {
        tr.point(sp);
        sp.x0 = x0;
        sp.xf = final_state;
        sp.nodes = nodes;
        if (tg) sp.ty = tg->y;
        sp.metrics = metrics;
        const hipError_t e = launch((hipStream_t)hip_stream);
        if (e != hipSuccess) return session_fail(s, CFX_EHIP, f + hipGetErrorString(e));
        return CFX_OK;
    }
    int rc = train_check(fn, s->model, s->scheme, s->m, s->B, s->P, s->Nmax, "instance", tr, s->err);
    if (rc != CFX_OK) return rc;
    if (tg && (rc = sweep_target_check(fn, tg, true, s->err)) != CFX_OK) return rc;
    if (x0)
        for (size_t i = 0; i < nx * B; ++i)
            if (!std::isfinite(x0[i])) return session_fail(s, CFX_EINVAL, f + "x0 is not finite");
    // staging slots 3..7: x0, xf, nodes, target, metrics
    double* d_x0 = x0 ? session_buf(s, fn, 3, nx * B, &rc) : nullptr;
    double* d_xf = session_buf(s, fn, 4, nx * B, &rc);
    double* d_nd = nodes ? session_buf(s, fn, 5, nn * nx * B, &rc) : nullptr;
    double* d_ty = tg ? session_buf(s, fn, 6, nt, &rc) : nullptr;
    double* d_mt = tg ? session_buf(s, fn, 7, (size_t)kSweepMetrics * B, &rc) : nullptr;
    if ((x0 && !d_x0) || !d_xf || (nodes && !d_nd) || (tg && (!d_ty || !d_mt))) return rc;
    hipStream_t st = s->stream;
    rc = tr.upload(s, fn, sp, [&]() -> int {
        if (d_x0) TRAIN_HIP(hipMemcpyAsync(d_x0, x0, nx * B * sizeof(double), hipMemcpyHostToDevice, st));
        if (d_ty) TRAIN_HIP(hipMemcpyAsync(d_ty, tg->y, nt * sizeof(double), hipMemcpyHostToDevice, st));
        return CFX_OK;
    });
    if (rc != CFX_OK) return rc;
    sp.x0 = d_x0;
    sp.xf = d_xf;
    sp.nodes = d_nd;
    sp.ty = d_ty;
    sp.metrics = d_mt;
    TRAIN_HIP(launch(st));
    TRAIN_HIP(hipMemcpyAsync(final_state, d_xf, nx * B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (d_nd) TRAIN_HIP(hipMemcpyAsync(nodes, d_nd, nn * nx * B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (d_mt)
        TRAIN_HIP(hipMemcpyAsync(metrics, d_mt, (size_t)kSweepMetrics * B * sizeof(double), hipMemcpyDeviceToHost, st));
    TRAIN_HIP(hipStreamSynchronize(st));
    return CFX_OK;
}

extern "C" int cfx_sweep_integrate(cfx_sweep* s, const cfx_sweep_trains* tr, const double* x0, double* final_state,
                                   double* nodes, uint32_t flags, void* hip_stream) {
    if (!s) return g_create_error = "cfx_sweep_integrate: NULL handle", CFX_EINVAL;
    if (!tr || !final_state) return session_fail(s, CFX_EINVAL, "cfx_sweep_integrate: trains or final_state is NULL");
    return sweep_run("cfx_sweep_integrate", s, tr, nullptr, x0, final_state, nodes, nullptr, flags, hip_stream);
}

extern "C" int cfx_sweep_score(cfx_sweep* s, const cfx_sweep_trains* tr, const cfx_sweep_target* tg, const double* x0,
                               double* final_state, double* metrics, uint32_t flags, void* hip_stream) {
    if (!s) return g_create_error = "cfx_sweep_score: NULL handle", CFX_EINVAL;
    if (!tr || !tg || !final_state || !metrics)
        return session_fail(s, CFX_EINVAL, "cfx_sweep_score: trains, target, final_state or metrics is NULL");
    // n_samples and sample_dt are host values with CFX_DEVICE too
    const int rc = sweep_target_check("cfx_sweep_score", tg, false, s->err);
    if (rc != CFX_OK) return rc;
    return sweep_run("cfx_sweep_score", s, tr, tg, x0, final_state, nullptr, metrics, flags, hip_stream);
}

// ------------------------------------------------------------------------------------------------------
// multi-train identification: E trains share the parameters of every start.  Force parameters (cfx_idm.h) and
// fatigue parameters (cfx_idfm.h) differ in the model family, the parameter list and the kernels.
// ------------------------------------------------------------------------------------------------------
struct IdmFamily {
    bool fatigue;       // the family's models
    const char* wrong;  // what a model of the other family is told (CFX_EUNSUPPORTED)
    int (*ids)(int model, int32_t n_id, const int32_t* ids, int32_t* col, std::string& msg);  // the parameter list
    size_t prefix;      // length of the name in that checker's messages, replaced by the caller's
};

static const IdmFamily kIdm = {false, "identification is not available for the fatigue models", id_check, 6};
static const IdmFamily kIdfm = {true, "fatigue-parameter identification is only available for the fatigue models",
                                idf_check, 7};

static const int kIdmRowsMax = 1 + CFX_ID_MAX_PARAMS + CFX_ID_MAX_PARAMS * (CFX_ID_MAX_PARAMS + 1) / 2;
static const int kIdfmRowsMax = 1 + CFX_IDF_MAX_PARAMS + CFX_IDF_MAX_PARAMS * (CFX_IDF_MAX_PARAMS + 1) / 2;

// Every argument check of a family's create (with_ids = false: no parameter list), forces and normal calls;
// tr != nullptr: the host arrays too.  The train rules are cfx_sweep_check's with the train in the instance's place,
// then target and weight.
static int idm_check(const char* fn, const IdmFamily& fam, int model, int scheme, int n_steps, int64_t B, int E, int P,
                     int Nmax, bool with_ids, int32_t n_id, const int32_t* ids, int32_t* col,
                     const cfx_idm_trains* tr, std::string& msg) {
    const std::string f = std::string(fn) + ": ";
    if (model < CFX_DING2003 || model > CFX_HMED2018_FATIGUE) return msg = f + "unknown model", CFX_EINVAL;
    if (is_fatigue(model) != fam.fatigue) return msg = f + fam.wrong, CFX_EUNSUPPORTED;
    if (E < 1) return msg = f + "n_trains must be positive", CFX_EINVAL;
    if (E > kMaxGridY) return msg = f + "n_trains must be <= 65535", CFX_EINVAL;
    if (with_ids) {
        std::string m2;
        const int rc = fam.ids(model, n_id, ids, col, m2);
        if (rc != CFX_OK) return msg = std::string(fn) + m2.substr(fam.prefix), rc;
    }
    if (B < 1) return msg = f + "n_steps, batch, max_pulses and max_shooting must be positive", CFX_EINVAL;
    const int rc = train_check(fn, model, scheme, n_steps, E, P, Nmax, "train", train_view(tr), msg);
    if (rc != CFX_OK || !tr) return rc;
    for (int pass = 0; pass < 2; ++pass) {
        const double* a = pass == 0 ? tr->target : tr->weight;
        if (!a) continue;
        for (int e = 0; e < E; ++e)
            for (int k = 0; k <= tr->n_shooting[e]; ++k) {
                const double v = a[(int64_t)k * E + e];
                if (!std::isfinite(v) || (pass == 1 && v < 0.0))
                    return msg = f + "train " + std::to_string(e) + ": node " + std::to_string(k) +
                                 (pass == 0 ? ": target is not finite" : ": weight must be finite and >= 0"),
                           CFX_EINVAL;
            }
    }
    return CFX_OK;
}

// What the forces and normal calls of both families do before the launch: the argument checks, then the device's
// view of the trains and of theta.  ip: the handle's parameters `base` with this call's columns and trains (the
// caller's own pointers with CFX_DEVICE, else the staging buffers after the upload); *TH the device theta; *st the
// stream to launch on.
template <class Params>
static int idm_begin(TrainSession* s, const Params& base, const IdmFamily& fam, const char* fn,
                     const cfx_idm_trains* trains, bool normal, int32_t n_id, const int32_t* ids, const double* theta,
                     uint32_t flags, void* hip_stream, Params& ip, const double** TH, hipStream_t* st) {
    const std::string f = std::string(fn) + ": ";
    if (!trains || !theta) return session_fail(s, CFX_EINVAL, f + "trains or theta is NULL");
    const TrainView tr = train_view(trains);
    if (tr.has_null(s->needs_value)) return session_fail(s, CFX_EINVAL, f + "a train array is NULL");
    if (normal && (!trains->target || !trains->weight))
        return session_fail(s, CFX_EINVAL, f + "target or weight is NULL");
    const bool dev = (flags & CFX_DEVICE) != 0;
    constexpr int kSlots = (int)(sizeof(base.col) / sizeof(base.col[0]));
    int32_t col[kSlots];
    // with device arrays only the creation arguments and the parameter list can be checked here
    int rc = idm_check(fn, fam, s->model, s->scheme, s->m, s->B, s->E, s->P, s->Nmax, true, n_id, ids, col,
                       dev ? nullptr : trains, s->err);
    if (rc != CFX_OK) return rc;
    ip = base;
    ip.n_id = n_id;
    for (int k = 0; k < kSlots; ++k) ip.col[k] = col[k];
    if (hipSetDevice(s->device) != hipSuccess) return session_fail(s, CFX_EHIP, f + "hipSetDevice failed");
    if (dev) {
        tr.point(ip);
        ip.target = trains->target;
        ip.weight = trains->weight;
        *TH = theta;
        *st = (hipStream_t)hip_stream;
        return CFX_OK;
    }
    const size_t B = (size_t)s->B, E = (size_t)s->E, nn = (size_t)s->Nmax + 1;
    for (size_t i = 0; i < (size_t)n_id * B; ++i)
        if (!std::isfinite(theta[i])) return session_fail(s, CFX_EINVAL, f + "theta is not finite");
    // staging slots 3..8: target, weight, theta, force, sens, cost | grad | gn | cost_per_train
    double* d_y = normal ? session_buf(s, fn, 3, nn * E, &rc) : nullptr;
    double* d_w = normal ? session_buf(s, fn, 4, nn * E, &rc) : nullptr;
    double* d_th = session_buf(s, fn, 5, (size_t)CFX_ID_MAX_PARAMS * B, &rc);
    if ((normal && (!d_y || !d_w)) || !d_th) return rc;
    hipStream_t q = s->stream;
    rc = tr.upload(s, fn, ip, [&]() -> int {
        if (d_y) TRAIN_HIP(hipMemcpyAsync(d_y, trains->target, nn * E * sizeof(double), hipMemcpyHostToDevice, q));
        if (d_w) TRAIN_HIP(hipMemcpyAsync(d_w, trains->weight, nn * E * sizeof(double), hipMemcpyHostToDevice, q));
        TRAIN_HIP(hipMemcpyAsync(d_th, theta, (size_t)n_id * B * sizeof(double), hipMemcpyHostToDevice, q));
        return CFX_OK;
    });
    if (rc != CFX_OK) return rc;
    ip.target = d_y;
    ip.weight = d_w;
    *TH = d_th;
    *st = q;
    return CFX_OK;
}

// What the forces calls of both families do around their launch: launch(F, S) (a CFX_* code) on the caller's arrays
// with CFX_DEVICE, else on the handle's buffers, followed by the copies back and the synchronisation.
template <class Launch>
static int idm_forces_staged(TrainSession* s, const char* fn, int32_t n_id, double* force, double* sens,
                             uint32_t flags, hipStream_t st, Launch&& launch) {
    int rc = CFX_OK;
    if (flags & CFX_DEVICE) return launch(force, sens);
    const size_t nf = (size_t)s->E * ((size_t)s->Nmax + 1) * (size_t)s->B, ns = nf * (size_t)n_id;
    double* d_f = session_buf(s, fn, 6, nf, &rc);
    double* d_s = sens ? session_buf(s, fn, 7, ns, &rc) : nullptr;
    if (!d_f || (sens && !d_s)) return rc;
    if ((rc = launch(d_f, d_s)) != CFX_OK) return rc;
    TRAIN_HIP(hipMemcpyAsync(force, d_f, nf * sizeof(double), hipMemcpyDeviceToHost, st));
    if (d_s) TRAIN_HIP(hipMemcpyAsync(sens, d_s, ns * sizeof(double), hipMemcpyDeviceToHost, st));
    TRAIN_HIP(hipStreamSynchronize(st));
    return CFX_OK;
}

// The same for the normal calls: launch(C, G, H, CPT).
template <class Launch>
static int idm_normal_staged(TrainSession* s, const char* fn, int32_t n_id, double* cost, double* grad, double* gn,
                             double* cost_per_train, uint32_t flags, hipStream_t st, Launch&& launch) {
    int rc = CFX_OK;
    if (flags & CFX_DEVICE) return launch(cost, grad, gn, cost_per_train);
    const size_t B = (size_t)s->B, n = (size_t)n_id, npk = n * (n + 1) / 2, E = (size_t)s->E;
    double* d_o = session_buf(s, fn, 8, (1 + n + npk + E) * B, &rc);
    if (!d_o) return rc;
    double *d_c = d_o, *d_g = d_o + B, *d_h = d_g + n * B, *d_p = cost_per_train ? d_h + npk * B : nullptr;
    if ((rc = launch(d_c, d_g, d_h, d_p)) != CFX_OK) return rc;
    TRAIN_HIP(hipMemcpyAsync(cost, d_c, B * sizeof(double), hipMemcpyDeviceToHost, st));
    TRAIN_HIP(hipMemcpyAsync(grad, d_g, n * B * sizeof(double), hipMemcpyDeviceToHost, st));
    TRAIN_HIP(hipMemcpyAsync(gn, d_h, npk * B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (d_p) TRAIN_HIP(hipMemcpyAsync(cost_per_train, d_p, E * B * sizeof(double), hipMemcpyDeviceToHost, st));
    TRAIN_HIP(hipStreamSynchronize(st));
    return CFX_OK;
}

// ------------------------------------------------------------------------------------------------------
// multi-train force-parameter identification (cfx_idm.h)
// ------------------------------------------------------------------------------------------------------
extern "C" int cfx_idm_check(int32_t model, int32_t scheme, int32_t n_steps, int64_t batch, int32_t n_trains,
                             int32_t max_pulses, int32_t max_shooting, int32_t n_id, const int32_t* param_ids,
                             const cfx_idm_trains* trains) {
    int32_t col[ID_SLOTS];
    return idm_check("cfx_idm_check", kIdm, model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting, true,
                     n_id, param_ids, col, trains, g_create_error);
}

extern "C" void cfx_idm_destroy(cfx_idm* s) { session_close(s); }

extern "C" const char* cfx_idm_last_error(const cfx_idm* s) { return session_error(s); }

extern "C" int cfx_idm_create(int32_t model, const cfx_constants* c, int32_t scheme, int32_t n_steps, int64_t batch,
                              int32_t n_trains, int32_t max_pulses, int32_t max_shooting, int32_t device,
                              cfx_idm** out) {
    if (!c || !out) return g_create_error = "cfx_idm_create: NULL argument", CFX_EINVAL;
    *out = nullptr;
    int rc = idm_check("cfx_idm_create", kIdm, model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting,
                       false, 0, nullptr, nullptr, nullptr, g_create_error);
    if (rc != CFX_OK) return rc;
    if (!(c->tauc > 0.0)) return g_create_error = "cfx_idm_create: tauc must be positive", CFX_EINVAL;
    rc = session_open("cfx_idm_create", model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting, device,
                      (size_t)n_trains * kIdmRowsMax * (size_t)batch, out);
    if (rc != CFX_OK) return rc;
    IdmParams& ip = (*out)->ip;
    ip.B = batch;
    ip.E = n_trains;
    ip.P = max_pulses;
    ip.Nmax = max_shooting;
    ip.m = n_steps;
    ip.inv_tauc = 1.0 / c->tauc;
    ip.mult = c->fl * c->fv + c->fp;
    ip.r0_km = c->r0_km_relationship;
    for (int k = 0; k < ID_SLOTS; ++k) ip.def[k] = 0.0;
    ip.def[ID_A] = is_pw(model) ? c->a_scale : c->a_rest;
    ip.def[ID_KM] = c->km_rest;
    ip.def[ID_TAU1] = c->tau1_rest;
    ip.def[ID_TAU2] = c->tau2;
    if (is_pw(model)) {
        ip.def[ID_P4] = c->pd0;
        ip.def[ID_P5] = c->pdt;
    }
    if (is_int(model)) {
        ip.def[ID_P4] = c->ar;
        ip.def[ID_P5] = c->bs;
        ip.def[ID_P6] = c->Is;
        ip.def[ID_P7] = c->cr;
    }
    return CFX_OK;
}

// slots 0..3 only: the 4-direction kernels
static int idm_dirs(const IdmParams& ip) {
    for (int k = 4; k < ID_SLOTS; ++k)
        if (ip.col[k] >= 0) return 8;
    return 4;
}

extern "C" int cfx_idm_forces(cfx_idm* s, const cfx_idm_trains* tr, int32_t n_id, const int32_t* param_ids,
                              const double* theta, double* force, double* sens, uint32_t flags, void* hip_stream) {
    const char* fn = "cfx_idm_forces";
    if (!s) return g_create_error = "cfx_idm_forces: NULL handle", CFX_EINVAL;
    if (!force) return session_fail(s, CFX_EINVAL, "cfx_idm_forces: force is NULL");
    IdmParams ip;
    const double* TH = nullptr;
    hipStream_t st = nullptr;
    const int rc = idm_begin(s, s->ip, kIdm, fn, tr, false, n_id, param_ids, theta, flags, hip_stream, ip, &TH, &st);
    if (rc != CFX_OK) return rc;
    return idm_forces_staged(s, fn, n_id, force, sens, flags, st, [&](double* F, double* S) -> int {
        TRAIN_HIP(launch_idm_sens(s->model, s->scheme, idm_dirs(ip), ip, TH, F, S, st));
        return CFX_OK;
    });
}

extern "C" int cfx_idm_normal(cfx_idm* s, const cfx_idm_trains* tr, int32_t n_id, const int32_t* param_ids,
                              const double* theta, double* cost, double* grad, double* gn, double* cost_per_train,
                              uint32_t flags, void* hip_stream) {
    const char* fn = "cfx_idm_normal";
    if (!s) return g_create_error = "cfx_idm_normal: NULL handle", CFX_EINVAL;
    if (!cost || !grad || !gn) return session_fail(s, CFX_EINVAL, "cfx_idm_normal: cost, grad or gn is NULL");
    IdmParams ip;
    const double* TH = nullptr;
    hipStream_t st = nullptr;
    const int rc = idm_begin(s, s->ip, kIdm, fn, tr, true, n_id, param_ids, theta, flags, hip_stream, ip, &TH, &st);
    if (rc != CFX_OK) return rc;
    const int d = idm_dirs(ip);
    return idm_normal_staged(s, fn, n_id, cost, grad, gn, cost_per_train, flags, st,
                             [&](double* C, double* G, double* H, double* CPT) -> int {
                                 TRAIN_HIP(launch_idm_normal(s->model, s->scheme, d, ip, TH, s->d_ws, C, G, H, CPT, st));
                                 return CFX_OK;
                             });
}

// ------------------------------------------------------------------------------------------------------
// multi-train fatigue-parameter identification (cfx_idfm.h)
// ------------------------------------------------------------------------------------------------------
extern "C" int cfx_idfm_check(int32_t model, int32_t scheme, int32_t n_steps, int64_t batch, int32_t n_trains,
                              int32_t max_pulses, int32_t max_shooting, int32_t n_id, const int32_t* param_ids,
                              const cfx_idm_trains* trains) {
    int32_t col[IDF_SLOTS];
    return idm_check("cfx_idfm_check", kIdfm, model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting, true,
                     n_id, param_ids, col, trains, g_create_error);
}

extern "C" void cfx_idfm_destroy(cfx_idfm* s) { session_close(s); }

extern "C" const char* cfx_idfm_last_error(const cfx_idfm* s) { return session_error(s); }

extern "C" int cfx_idfm_create(int32_t model, const cfx_constants* c, int32_t scheme, int32_t n_steps, int64_t batch,
                               int32_t n_trains, int32_t max_pulses, int32_t max_shooting, int32_t device,
                               cfx_idfm** out) {
    if (!c || !out) return g_create_error = "cfx_idfm_create: NULL argument", CFX_EINVAL;
    *out = nullptr;
    int rc = idm_check("cfx_idfm_create", kIdfm, model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting,
                       false, 0, nullptr, nullptr, nullptr, g_create_error);
    if (rc != CFX_OK) return rc;
    if (!(c->tauc > 0.0)) return g_create_error = "cfx_idfm_create: tauc must be positive", CFX_EINVAL;
    if (!(c->tau_fat > 0.0)) return g_create_error = "cfx_idfm_create: tau_fat must be positive", CFX_EINVAL;
    rc = session_open("cfx_idfm_create", model, scheme, n_steps, batch, n_trains, max_pulses, max_shooting, device,
                      (size_t)n_trains * kIdfmRowsMax * (size_t)batch, out);
    if (rc != CFX_OK) return rc;
    IdfmParams& fp = (*out)->fp;
    fp.B = batch;
    fp.E = n_trains;
    fp.P = max_pulses;
    fp.Nmax = max_shooting;
    fp.m = n_steps;
    fp.def[IDF_AA] = c->alpha_a;
    fp.def[IDF_AT] = c->alpha_tau1;
    fp.def[IDF_AK] = c->alpha_km;
    fp.def[IDF_TF] = c->tau_fat;
    fill_model_constants(model, c, fp);
    return CFX_OK;
}

extern "C" int cfx_idfm_forces(cfx_idfm* s, const cfx_idm_trains* tr, int32_t n_id, const int32_t* param_ids,
                               const double* theta, double* force, double* sens, uint32_t flags, void* hip_stream) {
    const char* fn = "cfx_idfm_forces";
    if (!s) return g_create_error = "cfx_idfm_forces: NULL handle", CFX_EINVAL;
    if (!force) return session_fail(s, CFX_EINVAL, "cfx_idfm_forces: force is NULL");
    IdfmParams fp;
    const double* TH = nullptr;
    hipStream_t st = nullptr;
    const int rc = idm_begin(s, s->fp, kIdfm, fn, tr, false, n_id, param_ids, theta, flags, hip_stream, fp, &TH, &st);
    if (rc != CFX_OK) return rc;
    return idm_forces_staged(s, fn, n_id, force, sens, flags, st, [&](double* F, double* S) -> int {
        TRAIN_HIP(launch_idfm_sens(s->model, s->scheme, fp, TH, F, S, st));
        return CFX_OK;
    });
}

extern "C" int cfx_idfm_normal(cfx_idfm* s, const cfx_idm_trains* tr, int32_t n_id, const int32_t* param_ids,
                               const double* theta, double* cost, double* grad, double* gn, double* cost_per_train,
                               uint32_t flags, void* hip_stream) {
    const char* fn = "cfx_idfm_normal";
    if (!s) return g_create_error = "cfx_idfm_normal: NULL handle", CFX_EINVAL;
    if (!cost || !grad || !gn) return session_fail(s, CFX_EINVAL, "cfx_idfm_normal: cost, grad or gn is NULL");
    IdfmParams fp;
    const double* TH = nullptr;
    hipStream_t st = nullptr;
    const int rc = idm_begin(s, s->fp, kIdfm, fn, tr, true, n_id, param_ids, theta, flags, hip_stream, fp, &TH, &st);
    if (rc != CFX_OK) return rc;
    return idm_normal_staged(s, fn, n_id, cost, grad, gn, cost_per_train, flags, st,
                             [&](double* C, double* G, double* H, double* CPT) -> int {
                                 TRAIN_HIP(launch_idfm_normal(s->model, s->scheme, fp, TH, s->d_ws, C, G, H, CPT, st));
                                 return CFX_OK;
                             });
}
#undef TRAIN_HIP
