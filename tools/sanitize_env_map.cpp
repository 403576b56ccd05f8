// sanitize_env_map.cpp — the host mirror of orbit_env_map and orbit_env_sample (orbit_amd/host/orbit_env_map.cpp over
// csrc/env_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: the sizes of
// tests/env_map_cases.py — sky 1 to 16, irradiance 1 to 8 (the odd sizes' NaN frame among them), prefiltered 1, 2, 5, 16 and
// 17 with 1, 2 and 5 levels, tables 1 to 17, sample counts 1 to 257, three deltas — over hand-built panoramas of 1 x 1, 2 x
// 1, 7 x 3 and 64 x 32 texels — constant, seeded noise, NaN, both infinities, negative texels, values near the largest float
// —, every panorama, cube, table and counter block in a heap buffer that ENDS at its last legal byte, so a tap or a texel
// past the end is a heap overflow; each product alone and from a caller's sky cube; the sampler over axis, edge and corner
// directions, zero and non-finite ones and lods from NaN to beyond the last level, float -> integer conversions that see
// them; then the jobs the calls must refuse.  Host code only; nothing of it runs on a device or inside Python.  From the
// repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_env_map.cpp orbit_amd/host/orbit_env_map.cpp -o /tmp/sanitize_env_map && /tmp/sanitize_env_map
// Exit status 0, one line of counters per case and the number of refused jobs is a clean run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../orbit_amd/csrc/env_common.h"
#include "orbit_env_map.hpp"
#include "orbit_host.hpp"
using namespace orbit;

template <class T>
static T *ending(size_t count) { // a heap block of exactly count elements (at least one byte, so NULL never means "made")
    return (T *)std::malloc(count ? count * sizeof(T) : 1);
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static float *make_panorama(uint32_t w, uint32_t h, int kind) {
    float *p = ending<float>((size_t)w * h * 4);
    uint32_t s = 12345u + (uint32_t)kind;
    for (size_t i = 0; i < (size_t)w * h * 4; i++) {
        const float r = (float)(lcg(s) >> 8) / 16777216.0f;
        p[i] = kind == 0 ? 0.75f : kind == 1 ? r * 4.0f : r;
    }
    if (kind == 2) { // hostile
        const float bad[] = {NAN, INFINITY, -INFINITY, -1.0f, 3.0e38f, -3.0e38f, 20000.0f, 1e-40f};
        for (size_t i = 0; i < (size_t)w * h * 4; i += 3) p[i] = bad[(i / 3) % 8];
    }
    return p;
}

struct Case {
    uint32_t pw, ph;
    int kind;
    uint32_t sky, irr, pre, levels, count, brdf, brdf_count;
    float delta;
};

static uint64_t refused = 0;
static void expect_refused(const OrbitEnvMap &j, const char *what) {
    try {
        raster::env_map(j);
    } catch (const Panic &) {
        refused++;
        return;
    }
    std::fprintf(stderr, "not refused: %s\n", what);
    std::exit(1);
}
static void expect_refused(const OrbitEnvSample &j, const char *what) {
    try {
        raster::env_sample_job(j);
    } catch (const Panic &) {
        refused++;
        return;
    }
    std::fprintf(stderr, "not refused: %s\n", what);
    std::exit(1);
}

int main() {
    const Case cases[] = {
        {1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0.5f},       {2, 1, 1, 2, 2, 2, 2, 2, 2, 2, 0.25f},        {7, 3, 2, 4, 3, 5, 5, 63, 16, 64, 0.5f},
        {64, 32, 1, 8, 5, 16, 1, 64, 17, 65, 0.5711987f}, {7, 3, 2, 16, 8, 17, 2, 65, 0, 0, 0.5f},   {2, 1, 2, 4, 2, 1, 5, 256, 0, 0, 0.5f},
        {64, 32, 1, 8, 3, 5, 2, 257, 0, 0, 0.25f},   {7, 3, 1, 16, 0, 16, 5, 7, 0, 0, 0.5f},       {7, 3, 2, 8, 0, 17, 5, 3, 0, 0, 0.5f},
        {1, 1, 0, 1, 0, 17, 1, 2, 0, 0, 0.5f},       {7, 3, 1, 4, 0, 2, 5, 64, 0, 0, 0.5f},        {2, 1, 1, 2, 5, 2, 1, 255, 0, 0, 0.5f},
    };
    for (const Case &c : cases) {
        OrbitEnvMapLayout lay;
        raster::env_layout(c.sky, c.irr, c.pre, c.levels, c.brdf, lay);
        float *pano = make_panorama(c.pw, c.ph, c.kind);
        uint16_t *sky = ending<uint16_t>(lay.sky_texels * 4), *irr = ending<uint16_t>(lay.irradiance_texels * 4);
        uint16_t *pre = ending<uint16_t>(lay.prefiltered_texels * 4), *brdf = ending<uint16_t>(lay.brdf_texels * 2);
        OrbitEnvMapStats *stats = ending<OrbitEnvMapStats>(1);
        OrbitEnvMap j{};
        j.equirect = pano, j.sky = sky, j.irradiance = c.irr ? irr : nullptr, j.prefiltered = c.pre ? pre : nullptr, j.brdf = c.brdf ? brdf : nullptr;
        j.stats = stats, j.equirect_w = c.pw, j.equirect_h = c.ph, j.sky_size = c.sky, j.irradiance_size = c.irr, j.prefiltered_size = c.pre;
        j.prefiltered_levels = c.levels, j.brdf_size = c.brdf, j.sample_count = c.count, j.sample_delta = c.delta, j.brdf_sample_count = c.brdf_count;
        uint64_t census[64] = {0};
        raster::env_map(j, census);
        const OrbitEnvMapStats whole = *stats;
        // each product alone from the caller's sky cube: the same bytes
        uint16_t *again = ending<uint16_t>((lay.irradiance_texels > lay.prefiltered_texels ? lay.irradiance_texels : lay.prefiltered_texels) * 4);
        OrbitEnvMap k = j;
        k.equirect = nullptr, k.brdf = nullptr, k.stats = nullptr;
        if (c.irr) {
            k.irradiance = again, k.prefiltered = nullptr;
            raster::env_map(k);
            if (std::memcmp(again, irr, lay.irradiance_texels * 8)) return std::fprintf(stderr, "irradiance alone differs\n"), 1;
        }
        if (c.pre) {
            k.irradiance = nullptr, k.prefiltered = again;
            raster::env_map(k);
            if (std::memcmp(again, pre, lay.prefiltered_texels * 8)) return std::fprintf(stderr, "prefiltered alone differs\n"), 1;
        }
        if (c.brdf) { // the table alone: no sky at all
            OrbitEnvMap t{};
            uint16_t *table = ending<uint16_t>(lay.brdf_texels * 2);
            t.brdf = table, t.brdf_size = c.brdf, t.brdf_sample_count = c.brdf_count;
            raster::env_map(t);
            if (std::memcmp(table, brdf, lay.brdf_texels * 4)) return std::fprintf(stderr, "table alone differs\n"), 1;
            std::free(table);
        }
        // the sampler over the cube just made
        const float parts[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.999f, -0.999f, 0.3f, 1e30f, 1e-30f, NAN, INFINITY, -INFINITY, 3.0e38f};
        const float lods[] = {0.0f, 0.5f, 1.25f, (float)lay.sky_levels - 1.0f, (float)lay.sky_levels + 3.0f, -1.0f, NAN, INFINITY, -INFINITY, 3.0e38f};
        const uint32_t np = sizeof(parts) / 4, nl = sizeof(lods) / 4, n = np * np * np * nl;
        float *dirs = ending<float>((size_t)n * 3), *lod = ending<float>(n), *rgb = ending<float>((size_t)n * 3);
        uint64_t *bad = ending<uint64_t>(1);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t d = i / nl;
            dirs[3 * i] = parts[d % np], dirs[3 * i + 1] = parts[(d / np) % np], dirs[3 * i + 2] = parts[d / (np * np)], lod[i] = lods[i % nl];
        }
        OrbitEnvSample s{};
        s.cube = sky, s.directions = dirs, s.lods = lod, s.rgb = rgb, s.bad_directions = bad, s.size = c.sky, s.levels = lay.sky_levels, s.n = n;
        raster::env_sample_job(s, census);
        std::printf("sky %u irr %u pre %u x %u table %u: nonfinite %llu %llu %llu %llu, bad directions %llu; sampler bad %llu of %u, corner taps %llu\n", c.sky,
                    c.irr, c.pre, c.levels, c.brdf, (unsigned long long)whole.sky_nonfinite, (unsigned long long)whole.irradiance_nonfinite,
                    (unsigned long long)whole.prefiltered_nonfinite, (unsigned long long)whole.brdf_nonfinite, (unsigned long long)whole.bad_directions,
                    (unsigned long long)*bad, n, (unsigned long long)census[30]);
        // the refused jobs, on this case's buffers
        OrbitEnvMap r = j;
        r.sky_size = c.sky + 1u == 2u ? 3u : c.sky * 2u + 1u, expect_refused(r, "sky_size not a power of two"), r = j;
        r.sky_size = 8192u, expect_refused(r, "sky_size above 4096"), r = j;
        r.flags = 1u, expect_refused(r, "flags"), r = j;
        r.equirect_w = 0u, expect_refused(r, "equirect_w 0"), r = j;
        r.sky = nullptr, expect_refused(r, "equirect without sky"), r = j;
        r.stats = (OrbitEnvMapStats *)((uint8_t *)stats + 4), expect_refused(r, "stats misaligned"), r = j;
        r.sky = sky + 1, expect_refused(r, "sky misaligned"), r = j;
        r.equirect = pano + 1, expect_refused(r, "equirect misaligned"), r = j;
        r.stats = (OrbitEnvMapStats *)sky, expect_refused(r, "stats is sky"), r = j;
        r.stats = (OrbitEnvMapStats *)(sky + 4 * (lay.sky_texels - 1)), expect_refused(r, "stats inside the sky cube's last texel"), r = j;
        if (c.irr) {
            for (const float d : {0.0f, -0.5f, 0.00005f, 0.0049f, (float)NAN, (float)INFINITY}) r.sample_delta = d, expect_refused(r, "sample_delta"), r = j;
            r.irradiance_size = 0u, expect_refused(r, "irradiance_size 0"), r = j;
            r.irradiance_size = 4097u, expect_refused(r, "irradiance_size above 4096"), r = j;
        }
        if (c.pre) {
            for (const uint32_t v : {0u, 65537u}) r.sample_count = v, expect_refused(r, "sample_count"), r = j;
            for (const uint32_t v : {0u, 14u}) r.prefiltered_levels = v, expect_refused(r, "prefiltered_levels"), r = j;
            r.prefiltered_size = 0u, expect_refused(r, "prefiltered_size 0"), r = j;
        }
        if (c.brdf) {
            for (const uint32_t v : {0u, 65537u}) r.brdf_sample_count = v, expect_refused(r, "brdf_sample_count"), r = j;
            r.brdf = (uint16_t *)((uint8_t *)brdf + 2), expect_refused(r, "brdf misaligned"), r = j;
        }
        r.sky = nullptr, r.equirect = nullptr, r.irradiance = nullptr, r.prefiltered = nullptr, r.brdf = nullptr, expect_refused(r, "no product");
        OrbitEnvSample q = s;
        q.size = 0u, expect_refused(q, "size 0"), q = s;
        q.levels = 0u, expect_refused(q, "levels 0"), q = s;
        q.levels = 14u, expect_refused(q, "levels 14"), q = s;
        q.cube = nullptr, expect_refused(q, "cube NULL"), q = s;
        q.rgb = nullptr, expect_refused(q, "rgb NULL"), q = s;
        q.cube = sky + 2, expect_refused(q, "cube misaligned"), q = s;
        q.flags = 4u, expect_refused(q, "flags"), q = s;
        q.rgb = lod, expect_refused(q, "rgb is lods"), q = s;
        q.bad_directions = (uint64_t *)(rgb + 3 * (size_t)n - 2), expect_refused(q, "counter inside rgb's end");
        std::free(pano), std::free(sky), std::free(irr), std::free(pre), std::free(brdf), std::free(stats), std::free(again);
        std::free(dirs), std::free(lod), std::free(rgb), std::free(bad);
    }
    std::printf("refused %llu jobs\n", (unsigned long long)refused);
    return 0;
}
