/* The cases of cast_check_main, shared with libcast_host.so so that the sanitised program's checksums can be compared with the plain
 * host build's: every kind in all four frames, from a reset-like state with tilted torsos and bent legs and from hostile ones (in the
 * position, the height, the quaternion, a joint angle and the items), at ray counts of one lane, of the wave's edge, of a second pass and
 * at the maximum, with every set of classes in turn, rays that are null, non-finite, huge, start inside the torso and under the ground,
 * links out of range, and each subset of the outputs. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/cast_core.h"

namespace cast_check {

constexpr int N_ENVS = 4, N_VARIANTS = 7, N_FRAMES = 4; /* reset-like, NaN, +inf, -inf, 1e20, denormal, aux[3] out of range */
constexpr int N_CASES = 6 * N_FRAMES * N_VARIANTS;
inline int n_cases() { return N_CASES; }

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
    /* (a NaN as one word: which NaN an operation yields is not part of the specification) */
    void eat_floats(const float *p, size_t n) {
        for (size_t j = 0; j < n; ++j) {
            uint32_t w = 0x7fc00000u;
            if (p[j] == p[j]) memcpy(&w, &p[j], 4);
            eat(&w, 4);
        }
    }
};

/* FNV-1a over the bytes of the four outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (N_FRAMES * N_VARIANTS), frame = (k / N_VARIANTS) % N_FRAMES, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_frame%d_variant%d", kind, frame, variant);
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
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.55f + 0.3f * rnd();
        const float yaw = 3.f * rnd(), tilt = 0.3f * rnd();
        st[3] = sinf(0.5f * tilt) * cosf(0.5f * yaw); st[4] = sinf(0.5f * tilt) * sinf(0.5f * yaw);
        st[5] = cosf(0.5f * tilt) * sinf(0.5f * yaw); st[6] = cosf(0.5f * tilt) * cosf(0.5f * yaw);
        for (int j = 0; j < 8; ++j) st[7 + j] = 1.2f * rnd();
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        aux[(size_t)e * HRL_AUX_STRIDE + 3] = e % 4;
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[k % 3] = h;
            if (e == 1) st[2] = h;
            if (e == 2) { items[(size_t)e * stride + 1] = h; st[7 + k % 8] = h; }
            if (e == 3) { items[(size_t)e * stride] = h; st[3 + k % 4] = h; }
        }
        if (variant == 6) aux[(size_t)e * HRL_AUX_STRIDE + 3] = e == 0 ? 1000 : (e == 1 ? -5 : (e == 2 ? 0x7fffffff : (int32_t)0x80000000));
    }
    hrl_cast_spec spec;
    if (hrl::cast::default_spec(&cfg, frame, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int counts[7] = {1, 63, 64, 65, 257, 1024, 16};
    const int R = counts[k % 7];
    spec.n_rays = R;
    spec.classes = (uint32_t)(k % 127) + 1u; /* 1..127: every bit of HRL_CHASE_ALL in turn */
    std::vector<float> rays((size_t)N_ENVS * R * 6);
    std::vector<int32_t> ray_link((size_t)R);
    for (int r = 0; r < R; ++r) ray_link[r] = r % 17 == 16 ? (r % 2 ? -1 : 13 + r) : r % 13;
    for (int e = 0; e < N_ENVS; ++e) {
        const float *st = &state[(size_t)e * HRL_STATE_STRIDE];
        for (int r = 0; r < R; ++r) {
            float *q = &rays[((size_t)e * R + r) * 6];
            const bool world = frame == HRL_CAST_WORLD;
            const float ox = world ? st[0] : 0.f, oy = world ? st[1] : 0.f, oz = world ? st[2] : 0.f;
            const float reach = frame == HRL_CAST_LINK ? 2.f : 8.f;
            q[0] = ox + 0.6f * rnd(); q[1] = oy + 0.6f * rnd(); q[2] = oz + 0.6f * rnd();
            q[3] = ox + reach * rnd(); q[4] = oy + reach * rnd(); q[5] = oz - reach * fabsf(rnd());
            switch (r % 23) {
                case 3: q[0] = ox; q[1] = oy; q[2] = oz; break;                         /* from the torso's centre */
                case 5: q[3] = q[0]; q[4] = q[1]; q[5] = q[2]; break;                   /* a null ray */
                case 7: q[r % 6] = hostile_value(1 + r % 5); break;                     /* a hostile number */
                case 11: q[2] = world ? -1.f : -3.f; break;                             /* from under the ground */
                case 13: q[3] = q[0]; q[4] = q[1]; break;                               /* vertical */
                case 17: q[5] = q[2]; q[4] = q[1]; break;                               /* along x */
                default: break;
            }
        }
    }
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = k % 11 == 10 ? nullptr : items.data(); b.aux = aux.data();
    const size_t n = (size_t)N_ENVS * R;
    std::vector<float> fraction(n, -3.f), point(3 * n, -5.f), normal(3 * n, -9.f);
    std::vector<int32_t> seg(n, -7);
    std::vector<uint8_t> mask(N_ENVS, 1);
    mask[k % N_ENVS] = (uint8_t)(k % 3 == 0 ? 0 : 2);
    hrl_cast_out out = {k % 5 == 4 ? nullptr : fraction.data(), k % 7 == 6 ? nullptr : seg.data(), k % 5 == 3 ? nullptr : point.data(), k % 5 == 2 ? nullptr : normal.data()};
    std::string why;
    const int rc = hrl::cast::cast_host_batch(&cfg, &b, &spec, rays.data(), k % 4 == 3 ? nullptr : ray_link.data(), k % 2 ? mask.data() : nullptr, &out, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    Fnv f;
    f.eat_floats(fraction.data(), n); f.eat(seg.data(), n * 4); f.eat_floats(point.data(), 3 * n); f.eat_floats(normal.data(), 3 * n);
    *checksum = f.h;
    return HRL_OK;
}

}  // namespace cast_check
