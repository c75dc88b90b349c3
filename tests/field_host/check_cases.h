/* The cases of field_check_main, shared with libfield_host.so so that the sanitised program's checksums can be compared with the plain
 * host build's: every kind in the three modes, from a reset-like state and from hostile ones (in the state and the items), at grid sizes
 * that are no multiple of 256 cells and at the maximum, under the three schedules. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/field_core.h"

namespace field_check {

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

/* FNV-1a over the bytes of the two outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (3 * N_VARIANTS), mode = (k / N_VARIANTS) % 3, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_mode%d_variant%d", kind, mode, variant);
    hrl_config cfg;
    if (hrl::default_config(kind, &cfg) != HRL_OK) return HRL_ERR_BAD_ARG;
    cfg.num_envs = N_ENVS;
    const int stride = hrl::items_stride(&cfg);
    std::vector<float> state((size_t)N_ENVS * HRL_STATE_STRIDE, 0.f), items((size_t)N_ENVS * stride, 0.f);
    std::vector<int32_t> aux((size_t)N_ENVS * HRL_AUX_STRIDE, 0);
    uint32_t lcg = 24680u + (uint32_t)k;
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
    hrl_field_spec spec;
    if (hrl::field::default_spec(&cfg, mode, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{64, 64}, {8, 8}, {24, 40}, {64, 8}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.sources |= HRL_FIELD_ROBOT;
    if (variant % 2) spec.margin = 0.f;
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = items.data(); b.aux = aux.data();
    const size_t n = (size_t)N_ENVS * spec.width * spec.height;
    std::vector<float> d(n, -1.f);
    std::vector<uint8_t> p(n, 255);
    hrl_field_out out = {d.data(), p.data()};
    std::string why;
    const int rc = hrl::field::field_host_batch(&cfg, &b, &spec, nullptr, &out, k % 3, nullptr, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    uint64_t h = 1469598103934665603ull;
    const uint8_t *pd = reinterpret_cast<const uint8_t *>(d.data());
    for (size_t j = 0; j < n * 4; ++j) { h ^= pd[j]; h *= 1099511628211ull; }
    for (size_t j = 0; j < n; ++j) { h ^= p[j]; h *= 1099511628211ull; }
    *checksum = h;
    return HRL_OK;
}

}  // namespace field_check
