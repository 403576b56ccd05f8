// sanitize_post_chain.cpp — the host mirrors of orbit_bloom and orbit_post_process (orbit_amd/host/orbit_post.cpp over
// csrc/post_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: the targets of
// tests/post_chain_cases.py (1 x 1 to 130 x 70) with hand-built colour planes — black, a checkerboard with a texel at
// 1e12, NaN and both infinities, values near the largest float — each plane, each mip chain and each output in a heap
// buffer that ENDS at its last legal byte, so a tap, a texel or a pixel past the end is a heap overflow; filter radii from
// 0 to 1e30 (taps far outside the level clamp at every edge, and float -> integer conversions see infinities), max_levels
// 1, 2 and 6, both render modes, both byte orders, each output alone; then the pack over every code and the jobs the calls
// must refuse.  Host code only; nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_post_chain.cpp orbit_amd/host/orbit_post.cpp \
//       -o /tmp/sanitize_post_chain && /tmp/sanitize_post_chain
// Exit status 0 and one line of counters per target is a clean run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../orbit_amd/csrc/post_common.h"
#include "orbit_host.hpp"
#include "orbit_post.hpp"
using namespace orbit;

int main() {
    const uint32_t targets[][2] = {{1, 1}, {2, 1}, {5, 3}, {1, 40}, {17, 9}, {64, 64}, {70, 33}, {130, 70}, {15, 17}, {16, 16}, {33, 31}, {32, 34}};
    const float radii[] = {0.0f, 0.003f, 0.025f, 0.5f, 3.0f, 1e30f};
    const uint32_t level_caps[] = {1u, 2u, 6u};
    uint64_t refused = 0;
    for (const auto &t : targets) {
        const uint32_t w = t[0], h = t[1];
        const size_t pixels = (size_t)w * h;
        float *color = (float *)std::malloc(pixels * 16); // malloc: 16-B aligned, ends at the last pixel
        uint64_t texels = 0, clamped = 0, nonfinite = 0, bloomed = 0, bad_pixels = 0;
        for (int image = 0; image < 4; image++) {
            for (size_t p = 0; p < pixels; p++) {
                const uint32_t x = (uint32_t)(p % w), y = (uint32_t)(p / w);
                float *c = color + 4 * p;
                c[3] = 1.0f;
                if (image == 0) c[0] = c[1] = c[2] = 0.0f;
                if (image == 1) c[0] = ((x + y) & 1u) ? 4.0f : 0.0f, c[1] = 0.5f, c[2] = ((x + y) & 1u) ? 0.0f : 8.0f;
                if (image == 2) c[0] = 0.25f * (float)(x % 7u), c[1] = 0.125f * (float)(y % 5u), c[2] = 1.0f;
                if (image == 3) c[0] = 3.0e38f, c[1] = 1.0e-40f, c[2] = (float)(x + 1u) * 1.0e37f;
            }
            if (image == 1) color[4 * (pixels / 2)] = 1.0e12f;
            if (image == 2) color[0] = NAN, color[4 * (pixels - 1) + 1] = INFINITY, color[4 * (pixels / 2) + 2] = -INFINITY;
            for (const uint32_t cap : level_caps)
                for (const float r : radii) {
                    OrbitBloomLayout lay;
                    raster::bloom_layout(w, h, cap, lay);
                    uint32_t *mips = (uint32_t *)std::malloc((size_t)lay.total_texels * 4);
                    OrbitBloomStats st;
                    OrbitBloom j{};
                    j.color = color, j.mips = mips, j.stats = &st, j.width = w, j.height = h, j.max_levels = cap;
                    j.threshold = image == 2 ? 1.0f : 0.0f, j.soft_threshold = image == 2 ? 0.5f : 0.0f, j.filter_radius = r;
                    raster::bloom(j);
                    texels += st.texels_written, clamped += st.clamped_texels, nonfinite += st.nonfinite_inputs;
                    for (uint32_t i = 0; i < lay.total_texels; i++) {
                        float rgb[3];
                        raster::bloom_unpack(mips[i], rgb);
                        if (!(std::fabs(rgb[0]) < INFINITY) || !(std::fabs(rgb[1]) < INFINITY) || !(std::fabs(rgb[2]) < INFINITY)) return 2; // B8
                    }
                    if (cap == 6u && (r == 0.003f || r == 1e30f))
                        for (int mode = 0; mode < 6; mode++) { // render modes, byte orders, each output alone, no bloom
                            float *ldr = mode == 4 ? nullptr : (float *)std::malloc(pixels * 16);
                            uint8_t *rgba8 = mode == 5 ? nullptr : (uint8_t *)std::malloc(pixels * 4);
                            OrbitPostStats ps;
                            OrbitPostProcess p{};
                            p.color = color, p.bloom = mode == 3 ? nullptr : mips, p.ldr = ldr, p.rgba8 = rgba8, p.stats = &ps;
                            p.exposure = mode == 2 ? 3.0e38f : 1.5f, p.bloom_intensity = mode == 2 ? 3.0e38f : 0.025f;
                            p.render_mode = mode == 1 ? 8u : 0u, p.width = w, p.height = h, p.flags = mode == 1 ? ORBIT_POST_BGRA : 0u;
                            raster::post_process(p);
                            bloomed += ps.bloom_pixels, bad_pixels += ps.nonfinite_pixels;
                            if (ldr)
                                for (size_t i = 0; i < 4 * pixels; i++)
                                    if (!(ldr[i] >= 0.0f && ldr[i] <= 1.0f)) return 3;
                            std::free(ldr), std::free(rgba8);
                        }
                    std::free(mips);
                }
        }
        std::printf("%3u x %-3u texels_written %llu clamped_texels %llu nonfinite_inputs %llu bloom_pixels %llu nonfinite_pixels %llu\n", w, h,
                    (unsigned long long)texels, (unsigned long long)clamped, (unsigned long long)nonfinite, (unsigned long long)bloomed,
                    (unsigned long long)bad_pixels);
        std::free(color);
    }
    // B7 over every code, one ulp either side, and the values no code holds
    uint64_t round_trips = 0;
    for (uint32_t word = 0; word < (1u << 11); word++)
        for (int neighbour = -1; neighbour <= 1; neighbour++) {
            float rgb[3], back[3];
            raster::bloom_unpack(word | (word << 11) | ((word >> 1) << 22), rgb);
            for (float &v : rgb) v = neighbour < 0 ? std::nextafter(v, -INFINITY) : neighbour > 0 ? std::nextafter(v, INFINITY) : v;
            bool c = false;
            raster::bloom_unpack(raster::bloom_pack(rgb, c), back);
            round_trips += back[0] == rgb[0] ? 1u : 0u;
        }
    const float odd[] = {0.0f, -0.0f, -1.0f, 1.0e-45f, 65024.0f, 64512.0f, 3.4e38f, INFINITY, -INFINITY, NAN};
    for (const float a : odd)
        for (const float b : odd) {
            const float rgb[3] = {a, b, a};
            bool c = false;
            (void)raster::bloom_pack(rgb, c);
            (void)raster::post_powc(a, b), (void)raster::post_exp2c(a * b);
        }
    // what the calls refuse: nothing is read or written
    OrbitBloom bad{};
    for (int k = 0; k < 6; k++) {
        alignas(16) float color[4] = {0, 0, 0, 1};
        uint32_t mip;
        bad = OrbitBloom{};
        bad.color = k == 0 ? nullptr : color, bad.mips = k == 1 ? nullptr : &mip, bad.width = k == 2 ? 0u : 1u, bad.height = 1u;
        bad.max_levels = k == 3 ? 7u : 1u, bad.filter_radius = k == 4 ? -1.0f : 0.0f, bad.flags = k == 5 ? 2u : 0u;
        try {
            raster::bloom(bad);
        } catch (const Panic &) {
            refused++;
        }
    }
    for (int k = 0; k < 4; k++) {
        alignas(16) float color[4] = {0, 0, 0, 1};
        uint32_t out;
        OrbitPostProcess p{};
        p.color = color, p.rgba8 = k == 0 ? nullptr : (uint8_t *)&out, p.width = 1u, p.height = k == 1 ? 0u : 1u;
        p.render_mode = k == 2 ? 7u : 0u, p.exposure = k == 3 ? NAN : 1.0f;
        try {
            raster::post_process(p);
        } catch (const Panic &) {
            refused++;
        }
    }
    std::printf("codes that round-trip (of %u x 3) %llu; jobs refused %llu of 10\n", 1u << 11, (unsigned long long)round_trips, (unsigned long long)refused);
    return refused == 10 ? 0 : 4;
}
