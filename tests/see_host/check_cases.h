/* The cases of see_check_main, shared with libsee_host.so so that the sanitised program's checksums can be compared with the plain host
 * build's: every kind in the three modes, from a reset-like state and from hostile ones (in the state and the items), at grid sizes that
 * are no multiple of 256 cells and at the maximum, with every set of occluders, slack, range and field of view in turn; in the world
 * mode with the memory, found full of arbitrary bytes, and a clear flag on some envs. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/see_core.h"

namespace see_check {

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

/* FNV-1a over the bytes of the three outputs; returns HRL_OK or the status of the launch */
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
    hrl_see_spec spec;
    if (hrl::see::default_spec(&cfg, mode, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{64, 64}, {8, 8}, {24, 40}, {64, 8}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.occluders = (uint32_t)(k % 32);
    if (k % 2) spec.slack = 0.f;
    if (k % 3 == 1) spec.max_range = 4.f;
    if (k % 4 >= 2) spec.fov_cos = k % 4 == 2 ? 0.5f : 0.f;
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = items.data(); b.aux = aux.data();
    const size_t cells = (size_t)spec.width * spec.height;
    std::vector<uint8_t> visible(N_ENVS * cells, 0x7B), seen(N_ENVS * cells), clear(N_ENVS);
    std::vector<int32_t> fresh(N_ENVS, -7);
    for (size_t i = 0; i < seen.size(); ++i) seen[i] = (uint8_t)((i * 7u + (uint32_t)k) % 5u == 0u ? (i & 0xffu) : 0u);
    for (int e = 0; e < N_ENVS; ++e) clear[e] = (uint8_t)((e + k) % 3 == 0 ? 1 + e : 0);
    const bool memory = mode == HRL_VIEW_WORLD;
    hrl_see_out out = {k % 5 == 4 && memory ? nullptr : visible.data(), memory ? seen.data() : nullptr, memory && k % 7 != 6 ? fresh.data() : nullptr};
    std::string why;
    const int rc = hrl::see::see_host_batch(&cfg, &b, &spec, k % 2 ? clear.data() : nullptr, nullptr, &out, nullptr, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    uint64_t h = 1469598103934665603ull;
    auto eat = [&h](const void *p, size_t bytes) {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (size_t j = 0; j < bytes; ++j) { h ^= q[j]; h *= 1099511628211ull; }
    };
    eat(visible.data(), visible.size()); eat(seen.data(), seen.size()); eat(fresh.data(), fresh.size() * 4);
    *checksum = h;
    return HRL_OK;
}

}  // namespace see_check
