/* The cases of chase_check_main, shared with libchase_host.so so that the sanitised program's checksums can be compared with the plain
 * host build's: every kind in both frames, from a reset-like state with tilted torsos and bent legs and from hostile ones (in the
 * position, the height, the quaternion, a joint angle and the items), at image sizes that leave waves idle, that end on a half-full pass
 * and at the maximum, with every set of classes, both target modes, pitches from straight down to above the horizon, yaws, distances,
 * ranges, tiles and fields of view in turn, and each subset of the outputs. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/chase_core.h"

namespace chase_check {

constexpr int N_ENVS = 4, N_VARIANTS = 7; /* reset-like, NaN, +inf, -inf, 1e20, denormal, aux[3] out of range */
constexpr int N_IMAGES = 6 * 2 * N_VARIANTS;
inline int n_cases() { return N_IMAGES; }

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

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void eat(const void *p, size_t bytes) {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (size_t j = 0; j < bytes; ++j) { h ^= q[j]; h *= 1099511628211ull; }
    }
};

/* FNV-1a over the bytes of the three outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (2 * N_VARIANTS), frame = (k / N_VARIANTS) % 2, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_frame%d_variant%d", kind, frame, variant);
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
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.55f + 0.3f * rnd();
        const float yaw = 3.f * rnd(), tilt = 0.3f * rnd();
        st[3] = sinf(0.5f * tilt) * cosf(0.5f * yaw); st[4] = sinf(0.5f * tilt) * sinf(0.5f * yaw);
        st[5] = cosf(0.5f * tilt) * sinf(0.5f * yaw); st[6] = cosf(0.5f * tilt) * cosf(0.5f * yaw);
        for (int j = 0; j < 8; ++j) st[7 + j] = 1.2f * rnd();
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        aux[(size_t)e * HRL_AUX_STRIDE + 3] = e % 4;
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[k % 2] = h;
            if (e == 1) st[2] = h;
            if (e == 2) { items[(size_t)e * stride + 1] = h; st[7 + k % 8] = h; }
            if (e == 3) { items[(size_t)e * stride] = h; st[3 + k % 4] = h; }
        }
        if (variant == 6) aux[(size_t)e * HRL_AUX_STRIDE + 3] = e == 0 ? 1000 : (e == 1 ? -5 : (e == 2 ? 0x7fffffff : (int32_t)0x80000000));
    }
    hrl_chase_spec spec;
    if (hrl::chase::default_spec(&cfg, frame, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{256, 256}, {16, 8}, {48, 24}, {64, 48}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.classes = (uint32_t)(k % 127) + 1u; /* 1..127: every bit of HRL_CHASE_ALL in turn */
    spec.target_mode = k % 2;
    spec.target_height = 0.2f * (float)(k % 3);
    const float pitches[6] = {-1.5707963267948966f, -1.48f, -1.05f, -0.52f, -0.17f, 0.35f}, yaw = 1.3f * (float)(k % 5);
    spec.pitch[0] = k % 6 == 0 ? 0.f : cosf(pitches[k % 6]); spec.pitch[1] = k % 6 == 0 ? -1.f : sinf(pitches[k % 6]);
    spec.yaw[0] = cosf(yaw); spec.yaw[1] = sinf(yaw);
    spec.distance = 1.5f * (float)(1 + k % 4);
    spec.tile = k % 3 == 2 ? 0.f : 0.5f * (float)(1 + k % 3);
    if (k % 3 == 1) spec.max_range = 5.f;
    if (k % 4 >= 2) { spec.tan_half_h = k % 4 == 2 ? 0.4f : 2.5f; spec.tan_half_v = 0.6f; }
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = k % 11 == 10 ? nullptr : items.data(); b.aux = aux.data();
    const size_t pixels = (size_t)spec.width * spec.height;
    std::vector<float> depth(N_ENVS * pixels, -3.f);
    std::vector<int32_t> seg(N_ENVS * pixels, -7);
    std::vector<uint8_t> rgb(N_ENVS * pixels * 3, 0x7B), mask(N_ENVS, 1);
    mask[k % N_ENVS] = (uint8_t)(k % 3 == 0 ? 0 : 2);
    hrl_chase_out out = {k % 5 == 4 ? nullptr : depth.data(), k % 7 == 6 ? nullptr : seg.data(), k % 5 == 3 ? nullptr : rgb.data()};
    std::string why;
    const int rc = hrl::chase::chase_host_batch(&cfg, &b, &spec, k % 2 ? mask.data() : nullptr, &out, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    Fnv f;
    f.eat(depth.data(), depth.size() * 4); f.eat(seg.data(), seg.size() * 4); f.eat(rgb.data(), rgb.size());
    *checksum = f.h;
    return HRL_OK;
}

}  // namespace chase_check
