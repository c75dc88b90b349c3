/* The cases of route_check_main, shared with libroute_host.so so that the sanitised program's checksums can be compared with the plain
 * host build's: every kind in the three modes, from a reset-like state and from hostile ones (in the state, the items and the starts),
 * at grid sizes that are no multiple of 256 cells and at the maximum, in the three frames, with both ways to decide `clear`. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/route_core.h"

namespace route_check {

constexpr int N_ENVS = 4, N_VARIANTS = 7; /* reset-like, NaN, +inf, -inf, 1e20, denormal, aux[3] out of range */
inline int n_cases() { return 6 * 3 * N_VARIANTS; }

inline float hostile_value(int variant) {
    switch (variant) {
        case 1: return __builtin_nanf("");
        case 2: return __builtin_inff();
        case 3: return -__builtin_inff();
        case 4: return 1e20f;
        case 5: return 1e-41f;
        default: return 0.f;
    }
}

/* FNV-1a over the bytes of the four outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (3 * N_VARIANTS), mode = (k / N_VARIANTS) % 3, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_mode%d_variant%d", kind, mode, variant);
    hrl_config cfg;
    if (hrl::default_config(kind, &cfg) != HRL_OK) return HRL_ERR_BAD_ARG;
    cfg.num_envs = N_ENVS;
    const int stride = hrl::items_stride(&cfg);
    std::vector<float> state((size_t)N_ENVS * HRL_STATE_STRIDE, 0.f), items((size_t)N_ENVS * stride, 0.f);
    std::vector<int32_t> aux((size_t)N_ENVS * HRL_AUX_STRIDE, 0);
    uint32_t lcg = 13579u + (uint32_t)k;
    auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f) * 2.f - 1.f; }; /* [-1, 1) */
    for (int e = 0; e < N_ENVS; ++e) {
        float *st = &state[(size_t)e * HRL_STATE_STRIDE];
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.55f;
        const float yaw = 3.f * rnd();
        st[5] = sinf(0.5f * yaw); st[6] = cosf(0.5f * yaw);
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        aux[(size_t)e * HRL_AUX_STRIDE + 3] = e % 4;
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[0] = h;
            if (e == 1) st[6] = h;
            if (e == 2) items[(size_t)e * stride + 1] = h;
            if (e == 3) { items[(size_t)e * stride] = h; st[1] = h; }
        }
        if (variant == 6) aux[(size_t)e * HRL_AUX_STRIDE + 3] = e == 0 ? 1000 : (e == 1 ? -5 : (e == 2 ? 0x7fffffff : (int32_t)0x80000000));
    }
    hrl_route_spec spec;
    if (hrl::route::default_spec(&cfg, mode, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{64, 64}, {8, 8}, {24, 40}, {64, 8}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.sources |= HRL_FIELD_ROBOT;
    if (variant % 2) spec.margin = 0.f;
    const int P = k % 2 ? 64 : 5, K = k % 3 == 0 ? 2 : (k % 3 == 1 ? 7 : 32);
    spec.n_starts = P; spec.max_waypoints = K; spec.frame = (k / 2) % 3;
    std::vector<float> starts((size_t)N_ENVS * P * 2);
    const float reach = spec.frame == HRL_PROBE_WORLD ? 9.f : 5.f;
    for (size_t i = 0; i < starts.size(); ++i) starts[i] = reach * rnd();
    if (variant >= 1 && variant <= 5) starts[3] = starts[2 * P] = hostile_value(variant);
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = items.data(); b.aux = aux.data();
    const size_t n = (size_t)N_ENVS * P;
    std::vector<float> w(n * K * 2, -1.f), len(n, -1.f);
    std::vector<int32_t> cnt(n, -7), cells(n * K, -7);
    hrl_route_out out = {w.data(), cnt.data(), len.data(), cells.data()};
    std::string why;
    const int rc = hrl::route::route_host_batch(&cfg, &b, &spec, k % 5 == 4 ? nullptr : starts.data(), nullptr, &out, k % 2, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    uint64_t h = 1469598103934665603ull;
    auto eat = [&h](const void *p, size_t bytes) {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (size_t j = 0; j < bytes; ++j) { h ^= q[j]; h *= 1099511628211ull; }
    };
    eat(w.data(), w.size() * 4); eat(cnt.data(), cnt.size() * 4); eat(len.data(), len.size() * 4); eat(cells.data(), cells.size() * 4);
    *checksum = h;
    return HRL_OK;
}

}  // namespace route_check
