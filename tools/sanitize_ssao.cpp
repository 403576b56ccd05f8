// sanitize_ssao.cpp — the host mirror of orbit_ssao (orbit_amd/host/orbit_ssao.cpp over csrc/ssao_common.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: the SSAO sizes of tests/ssao_cases.py (1 x
// 1 to 70 x 33), each with the screen at that size, at twice it and at twice it plus one, over hand-built depth planes —
// uncovered, a plane, a floor with a box, NaN, both infinities and negative texels, values near the largest float —, every
// plane, table and output in a heap buffer that ENDS at its last legal byte, so a tap, a texel or a pixel past the end is a
// heap overflow; the wrapped pixel 0xFFFFFFFF of A1 and positions beyond the grid, float -> integer conversions that see
// infinities and NaN, noise sizes 1, 3, 4 and 64 (all-zero and -128 texels among them), sample tables of 1, 64, 100 and 256
// texels, sample counts 1 to 64, radii 0 to 3e38, each legal output subset; then the jobs the call must refuse.  Host
// code only; nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_ssao.cpp orbit_amd/host/orbit_ssao.cpp -o /tmp/sanitize_ssao && /tmp/sanitize_ssao
// Exit status 0 and one line of counters per size is a clean run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../orbit_amd/csrc/ssao_common.h"
#include "orbit_host.hpp"
#include "orbit_ssao.hpp"
using namespace orbit;

static void make_camera(uint32_t w, uint32_t h, float *proj, float *inv) { // fov 90 degrees, near 0.01, reverse-z, infinite far plane
    const float aspect = (float)w / (float)h, near = 0.01f;
    std::memset(proj, 0, 64), std::memset(inv, 0, 64);
    proj[0] = 1.0f / aspect, proj[5] = 1.0f, proj[11] = -1.0f, proj[14] = near;
    inv[0] = aspect, inv[5] = 1.0f, inv[11] = 1.0f / near, inv[14] = -1.0f;
}

int main() {
    const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {1, 9}, {5, 3}, {7, 7}, {8, 8}, {9, 9}, {15, 17}, {16, 16}, {17, 15}, {33, 31}, {70, 33}};
    const uint32_t noise_sizes[] = {4u, 1u, 3u, 64u}, sample_sizes[] = {64u, 1u, 100u, 256u}, counts[] = {32u, 1u, 2u, 31u, 33u, 64u};
    const float radii[][2] = {{0.1f, 0.5f}, {0.0f, 0.0f}, {1.0f, 1.0f}, {3.0e38f, 3.0e38f}};
    uint64_t refused = 0;
    for (const auto &s : sizes) {
        const uint32_t w = s[0], h = s[1];
        uint64_t in_range = 0, nonfinite = 0, unoccluded = 0, runs = 0;
        for (int scale = 0; scale < 3; scale++) {
            const uint32_t sw = scale == 0 ? w : 2u * w + (scale == 2 ? 1u : 0u), sh = scale == 0 ? h : 2u * h + (scale == 2 ? 1u : 0u);
            const size_t pixels = (size_t)sw * sh;
            float *depth = (float *)std::malloc(pixels * 4); // ends at the last texel
            for (int image = 0; image < 5; image++) {
                for (size_t p = 0; p < pixels; p++) {
                    const uint32_t x = (uint32_t)(p % sw), y = (uint32_t)(p / sw);
                    float d = 0.0f;
                    if (image == 1) d = 0.002f;
                    if (image == 2) d = (x >= sw / 3u && x < 2u * sw / 3u && y >= sh / 3u) ? 0.01f / 3.0f : 0.01f / (2.0f + 6.0f * (1.0f - ((float)y + 0.5f) / (float)sh));
                    if (image == 3) d = 0.01f / (4.0f + (float)((x * 7u + y * 3u) % 11u) * 0.2f);
                    if (image == 4) d = ((x + y) & 1u) ? 3.0e38f : 1.0e-40f;
                    depth[p] = d;
                }
                if (image == 3) depth[0] = NAN, depth[pixels - 1] = INFINITY, depth[pixels / 2] = -0.002f, depth[pixels / 3] = -INFINITY;
                for (int v = 0; v < 4; v++) { // the table sizes and contents, the sample counts and the radii, varied together
                    const uint32_t ns = noise_sizes[(v + image) % 4], ms = sample_sizes[(v + scale) % 4];
                    int8_t *noise = (int8_t *)std::malloc((size_t)ns * ns * 2);
                    uint8_t *samples = (uint8_t *)std::malloc((size_t)ms * 4);
                    for (uint32_t i = 0; i < ns * ns * 2u; i++) noise[i] = (int8_t)(v == 1 ? 0 : v == 2 ? -128 : (int)((i * 37u + 11u) % 255u) - 127);
                    if (v == 3) noise[0] = noise[1] = 0;
                    for (uint32_t i = 0; i < ms * 4u; i++) samples[i] = (uint8_t)((i * 73u + 5u) & 255u);
                    for (int subset = 0; subset < 3; subset++) {
                        const uint32_t count = counts[(v + subset + image) % 6];
                        uint8_t *raw = (uint8_t *)std::malloc((size_t)w * h), *blurred = subset >= 1 ? (uint8_t *)std::malloc((size_t)w * h) : nullptr;
                        float *ao = subset >= 2 ? (float *)std::malloc(pixels * 4) : nullptr;
                        OrbitSsaoStats st;
                        uint64_t census[19];
                        OrbitSsao j{};
                        j.depth = depth, j.noise = noise, j.samples = samples, j.raw = raw, j.blurred = blurred, j.ao_pixel = ao, j.stats = subset == 1 ? nullptr : &st;
                        make_camera(sw, sh, j.projection, j.inverse_projection);
                        j.screen_w = sw, j.screen_h = sh, j.ssao_w = w, j.ssao_h = h, j.noise_size = ns, j.samples_size = ms, j.sample_count = count;
                        j.min_radius = radii[(v + subset) % 4][0], j.max_radius = radii[(v + subset) % 4][1];
                        raster::ssao(j, subset == 0 ? census : nullptr);
                        runs++;
                        if (j.stats) {
                            if (st.pixels != w * h) return 2;
                            in_range += st.samples_in_range, nonfinite += st.nonfinite_pixels, unoccluded += st.unoccluded_pixels;
                        }
                        if (ao)
                            for (size_t p = 0; p < pixels; p++)
                                if (!(ao[p] >= 0.0f && ao[p] <= 1.0f)) return 3; // bytes / 255 under weights that sum to 1, give or take a rounding
                        std::free(raw), std::free(blurred), std::free(ao);
                    }
                    std::free(noise), std::free(samples);
                }
            }
            std::free(depth);
        }
        std::printf("%3u x %-3u runs %llu samples_in_range %llu nonfinite_pixels %llu unoccluded_pixels %llu\n", w, h, (unsigned long long)runs,
                    (unsigned long long)in_range, (unsigned long long)nonfinite, (unsigned long long)unoccluded);
    }
    // the pieces on values no frame holds
    const float odd[] = {0.0f, -0.0f, -1.0f, 1.0e-45f, 1.0f, 3.4e38f, INFINITY, -INFINITY, NAN};
    for (const float a : odd)
        for (const float b : odd) {
            const float q[3] = {a, b, a};
            bool nf;
            (void)raster::ssao_in_range(q), (void)raster::ssao_range_check(a, b, a), (void)raster::ssao_byte(a * b, nf);
            (void)raster::bloom_axis(a, 7u), (void)raster::ssao_smoothstep(a, b, a);
        }
    // what the call refuses: nothing is read or written
    for (int k = 0; k < 12; k++) {
        float depth[1] = {0.002f}, ao[1];
        int8_t noise[2] = {1, 1};
        alignas(4) uint8_t samples[4] = {0, 0, 0, 0};
        uint8_t raw[1], blurred[1];
        OrbitSsao j{};
        j.depth = k == 0 ? nullptr : depth, j.noise = k == 1 ? nullptr : noise, j.samples = samples;
        j.raw = k == 2 ? nullptr : raw, j.blurred = k == 3 ? nullptr : blurred, j.ao_pixel = ao;
        make_camera(1, 1, j.projection, j.inverse_projection);
        j.screen_w = k == 4 ? 0u : 1u, j.screen_h = 1u, j.ssao_w = k == 5 ? 2u : 1u, j.ssao_h = 1u;
        j.noise_size = k == 6 ? 65u : 1u, j.samples_size = k == 7 ? 0u : 1u, j.sample_count = k == 8 ? 65u : 1u;
        j.min_radius = k == 9 ? -1.0f : 0.1f, j.max_radius = k == 10 ? NAN : 0.5f, j.flags = k == 11 ? 1u : 0u;
        try {
            raster::ssao(j);
        } catch (const Panic &) {
            refused++;
        }
    }
    std::printf("jobs refused %llu of 12\n", (unsigned long long)refused);
    return refused == 12 ? 0 : 4;
}
