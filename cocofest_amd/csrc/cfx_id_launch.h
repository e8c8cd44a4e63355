// cfx_id_launch.h — the model / scheme / D switch of the four identification launchers (cfx_inst_ident.hip,
// cfx_inst_identf.hip, cfx_inst_idm.hip, cfx_inst_idfm.hip).  go(model, scheme[, d]) receives the template arguments
// as std::integral_constant tags and launches that instantiation; a combination without kernels is
// hipErrorInvalidValue.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "cfx_kernels.h"

namespace cfx {

template <int V>
using IdTag = std::integral_constant<int, V>;

template <class Go>
hipError_t id_by_scheme(int scheme, Go&& go) {
    switch (scheme) {
        case 1: return go(IdTag<1>{});
        case 2: return go(IdTag<2>{});
        case 4: return go(IdTag<4>{});
        default: return hipErrorInvalidValue;
    }
}

// force family: D = 4 serves any subset of the first four slots, D = 8 everything else (Ding2003 has only four)
template <class Go>
hipError_t id_dispatch(int model, int scheme, int d, Go&& go) {
    if (d != 4 && d != 8) return hipErrorInvalidValue;
    return id_by_scheme(scheme, [&](auto S) {
        switch (model) {
            case M_D03: return d == 4 ? go(IdTag<M_D03>{}, S, IdTag<4>{}) : hipErrorInvalidValue;
            case M_D07: return d == 4 ? go(IdTag<M_D07>{}, S, IdTag<4>{}) : go(IdTag<M_D07>{}, S, IdTag<8>{});
            case M_H18: return d == 4 ? go(IdTag<M_H18>{}, S, IdTag<4>{}) : go(IdTag<M_H18>{}, S, IdTag<8>{});
            default: return hipErrorInvalidValue;
        }
    });
}

// fatigue family
template <class Go>
hipError_t idf_dispatch(int model, int scheme, Go&& go) {
    return id_by_scheme(scheme, [&](auto S) {
        switch (model) {
            case M_D03F: return go(IdTag<M_D03F>{}, S);
            case M_D07F: return go(IdTag<M_D07F>{}, S);
            case M_H18F: return go(IdTag<M_H18F>{}, S);
            default: return hipErrorInvalidValue;
        }
    });
}

// multi-train families: one block of `block` threads (one wave) per 64 starts of one train
inline dim3 id_train_grid(int64_t B, int E, int block) { return dim3((unsigned)((B + block - 1) / block), (unsigned)E); }

}  // namespace cfx
