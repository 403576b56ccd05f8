// sanitize_visibility_surface.cpp — the host mirror of orbit_raster_visibility and orbit_visibility_surface
// (orbit_amd/host/orbit_raster.cpp over csrc/raster_common.h and csrc/surface_common.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone host program: one drawn buffer, then the same buffer with a stale and a
// foreign word written into it.  Host code only; nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_visibility_surface.cpp orbit_amd/host/orbit_raster.cpp -o /tmp/sanitize_surface \
//       && /tmp/sanitize_surface
// Exit status 0 and two lines of counters (121 written; then 121 written, 1 foreign, 1 stale, status -9) is a clean run.
#include <cstdio>
#include <cstring>
#include <vector>
#include "orbit_raster.hpp"
#include "orbit_host.hpp"
using namespace orbit;
int main() {
    const uint32_t W = 65, H = 9;
    float vp[16] = {0};
    vp[0] = 2.0f / W, vp[5] = -2.0f / H, vp[10] = 1, vp[12] = -1, vp[13] = 1, vp[15] = 1;
    std::vector<float> pos = {3.3f, 1.2f, 0.5f, 9.1f, 7.7f, 0.5f, 40.6f, 2.4f, 0.5f, 50.25f, 2.25f, 0.25f, 50.25f, 2.95f, 0.25f, 50.95f, 2.25f, 0.25f};
    std::vector<uint32_t> data = {0, 1, 2, 3, 4, 5, 0, 0};
    uint8_t corners[8] = {0, 1, 2, 3, 4, 5, 0, 0};
    std::memcpy(&data[6], corners, 8);
    std::vector<uint32_t> cmds = {1, 6, 1, 24, 0, 0, 0, 0};
    std::vector<OrbitEntityData> ent(1);
    std::memset(ent.data(), 0, sizeof(OrbitEntityData));
    for (int i = 0; i < 4; i++) ent[0].model_matrix[5 * i] = 1.0f;
    std::vector<uint64_t> vis(W * H);
    raster::HostJob j{};
    j.draw_commands = cmds.data(), j.max_commands = 1, j.meshlet_data = data.data(), j.meshlet_data_words = data.size();
    j.vertices = (const uint8_t *)pos.data(), j.vertex_count = 6, j.vertex_stride = 12, j.position_offset = 0;
    j.entity_data = ent.data(), j.entity_count = 1, j.view_proj = vp, j.width = W, j.height = H, j.flags = ORBIT_RASTER_CLEAR;
    OrbitRasterStats rs;
    raster::raster_visibility(j, vis.data(), 0, &rs, nullptr);
    for (int tamper = 0; tamper < 2; tamper++) {
        if (tamper) vis[0] = vis[2 * W + 10] | 200u, vis[1] = (0x3f000000ull << 32) | (5u << 8); // t >= nt; a foreign id
        std::vector<float> bary(2 * W * H), grad(4 * W * H);
        std::vector<uint32_t> tri(4 * W * H);
        OrbitSurfaceStats st;
        OrbitVisibilitySurface s{};
        s.visibility = vis.data(), s.draw_commands = cmds.data(), s.meshlet_data = data.data(), s.vertices = pos.data();
        s.entity_data = ent.data(), s.bary = bary.data(), s.grad = grad.data(), s.triangle = tri.data(), s.stats = &st;
        s.meshlet_data_words = data.size(), s.vertex_count = 6, s.max_commands = 1, s.entity_count = 1, s.vertex_stride = 12;
        s.width = W, s.height = H, s.flags = ORBIT_SURFACE_CLEAR;
        std::memcpy(s.view_proj, vp, 64);
        int32_t status = 7;
        raster::visibility_surface(s, &status);
        std::printf("fragments %u: covered %u written %u foreign %u stale %u degenerate %u status %d\n", rs.fragments, st.covered_pixels,
                    st.written_pixels, st.foreign_pixels, st.stale_pixels, st.degenerate_pixels, status);
        if (st.covered_pixels != st.written_pixels + st.foreign_pixels + st.stale_pixels + st.unsupported_pixels) return 1;
    }
    return 0;
}
