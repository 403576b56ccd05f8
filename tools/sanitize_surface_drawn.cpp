// sanitize_surface_drawn.cpp — the host mirror of orbit_raster_visibility with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD
// and of orbit_visibility_surface_drawn (orbit_amd/host/orbit_raster.cpp over csrc/raster_common.h and csrc/surface_common.h)
// under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: one cut triangle whose piece
// (b, c, Q) is narrow and whose piece (b, Q, P) is wide (tests/surface_drawn_cases.py's cut_with_a_wide_piece_65x9), read
// with both flags, with the clip flag alone and with none; then the same buffer with a flipped depth bit and a foreign
// word.  Host code only; nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_surface_drawn.cpp orbit_amd/host/orbit_raster.cpp -o /tmp/sanitize_surface_drawn \
//       && /tmp/sanitize_surface_drawn
// Exit status 0 and four lines of counters is a clean run: clean, flags 40: 558 covered, 558 written, 558 cut, 381 wide;
// flags 8: the wide piece's 381 pixels unsupported; flags 0: all 558 unsupported; tampered, flags 40: 1 stale (status -9)
// and 1 foreign.
#include <cstdio>
#include <cstring>
#include <vector>
#include "orbit_raster.hpp"
#include "orbit_host.hpp"
using namespace orbit;
int main() {
    const uint32_t W = 65, H = 9;
    float vp[16] = {0};
    vp[0] = 1, vp[5] = 1, vp[11] = 1, vp[14] = 0.1f; // clip = (x, y, 0.1, z)
    std::vector<float> pos = {300.0f, 0.0f, 0.05f, -0.18f, -0.18f, 0.2f, -0.09f, 0.09f, 0.10002f};
    std::vector<uint32_t> data = {0, 1, 2, 0};
    const uint8_t corners[4] = {0, 1, 2, 0};
    std::memcpy(&data[3], corners, 4);
    std::vector<uint32_t> cmds = {1, 3, 1, 12, 0, 0, 0, 0};
    std::vector<OrbitEntityData> ent(1);
    std::memset(ent.data(), 0, sizeof(OrbitEntityData));
    for (int i = 0; i < 4; i++) ent[0].model_matrix[5 * i] = 1.0f;
    std::vector<uint64_t> vis(W * H);
    raster::HostJob j{};
    j.draw_commands = cmds.data(), j.max_commands = 1, j.meshlet_data = data.data(), j.meshlet_data_words = data.size();
    j.vertices = (const uint8_t *)pos.data(), j.vertex_count = 3, j.vertex_stride = 12, j.position_offset = 0;
    j.entity_data = ent.data(), j.entity_count = 1, j.view_proj = vp, j.width = W, j.height = H;
    j.flags = ORBIT_RASTER_CLEAR | ORBIT_RASTER_CULL_NONE | ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD;
    OrbitRasterStats rs;
    raster::raster_visibility(j, vis.data(), 0, &rs, nullptr);
    const uint32_t both = ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD;
    const uint32_t reads[4][2] = {{0, both}, {0, ORBIT_RASTER_CLIP_NEAR}, {0, 0}, {1, both}}; // (tampered, raster_flags)
    for (const auto &read : reads) {
        std::vector<uint64_t> buf = vis;
        if (read[0]) buf[4 * W + 30] ^= 1ull << 32, buf[0] = (0x3f000000ull << 32) | (5u << 8); // a depth bit; a foreign id
        std::vector<float> bary(2 * W * H), grad(4 * W * H);
        std::vector<uint32_t> tri(4 * W * H);
        OrbitSurfaceStats st;
        OrbitVisibilitySurface s{};
        s.visibility = buf.data(), s.draw_commands = cmds.data(), s.meshlet_data = data.data(), s.vertices = pos.data();
        s.entity_data = ent.data(), s.bary = bary.data(), s.grad = grad.data(), s.triangle = tri.data(), s.stats = &st;
        s.meshlet_data_words = data.size(), s.vertex_count = 3, s.max_commands = 1, s.entity_count = 1, s.vertex_stride = 12;
        s.width = W, s.height = H, s.flags = ORBIT_SURFACE_CLEAR;
        std::memcpy(s.view_proj, vp, 64);
        int32_t status = 7;
        raster::visibility_surface_drawn(s, read[1], &status);
        std::printf("fragments %u, flags %u: covered %u written %u foreign %u unsupported %u stale %u cut %u wide %u status %d\n", rs.fragments,
                    read[1], st.covered_pixels, st.written_pixels, st.foreign_pixels, st.unsupported_pixels, st.stale_pixels, st.cut_pixels,
                    st.wide_pixels, status);
        if (st.covered_pixels != st.written_pixels + st.foreign_pixels + st.stale_pixels + st.unsupported_pixels) return 1;
        if (read[1] == both && !read[0] && (st.written_pixels != st.covered_pixels || st.wide_pixels == 0 || st.wide_pixels >= st.cut_pixels)) return 1;
        if (read[1] == both && read[0] && (st.stale_pixels != 1 || st.foreign_pixels != 1 || status != ORBIT_E_RANGE)) return 1;
    }
    return 0;
}
