// sanitize_surface_fragments.cpp — the host mirror's chain orbit_raster_visibility -> orbit_visibility_surface_drawn ->
// orbit_surface_fragments (orbit_amd/host/orbit_raster.cpp over csrc/raster_common.h, csrc/surface_common.h and
// csrc/fragment_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: the cut
// triangle of tools/sanitize_surface_drawn.cpp drawn and read with both flags, its three vertices as 32-B MeshVertex rows
// in a heap buffer that ENDS with the last row's tangent (92 bytes) and its meshlet in a heap buffer that ENDS with the
// record's material_index (30 bytes), so a read of a whole row or record is a heap overflow; then the same buffers with a
// triangle record naming vertex 3 (= vertex_count), one naming entity 1 (= entity_count), one left out (0xFFFFFFFF) and a
// foreign word.  Host code only; nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_surface_fragments.cpp orbit_amd/host/orbit_raster.cpp -o /tmp/sanitize_surface_fragments \
//       && /tmp/sanitize_surface_fragments
// Exit status 0 and two lines of counters is a clean run: clean: 558 covered, 558 written, status 0; tampered: 559 covered, 2 stale
// (status -9), 1 unshaded, 1 foreign, 555 written.
#include <cstdio>
#include <cstdlib>
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
    std::vector<uint32_t> cmds = {1, 3, 1, 12, 0, 0, 0, 0}; // count; one command: entity 0, meshlet_index 0
    std::vector<OrbitEntityData> ent(1);
    std::memset(ent.data(), 0, sizeof(OrbitEntityData));
    for (int i = 0; i < 4; i++) ent[0].model_matrix[5 * i] = 1.0f, ent[0].normal_matrix[5 * i] = 1.0f;
    ent[0].normal_matrix[4] = 0.25f;
    std::vector<uint64_t> vis(W * H);
    raster::HostJob j{};
    j.draw_commands = cmds.data(), j.max_commands = 1, j.meshlet_data = data.data(), j.meshlet_data_words = data.size();
    j.vertices = (const uint8_t *)pos.data(), j.vertex_count = 3, j.vertex_stride = 12, j.position_offset = 0;
    j.entity_data = ent.data(), j.entity_count = 1, j.view_proj = vp, j.width = W, j.height = H;
    j.flags = ORBIT_RASTER_CLEAR | ORBIT_RASTER_CULL_NONE | ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD;
    OrbitRasterStats rs;
    raster::raster_visibility(j, vis.data(), 0, &rs, nullptr);
    // the same vertices as MeshVertex rows, the last one cut behind its tangent; the meshlet cut behind its material
    const size_t rows_bytes = 3 * 32 - 4, meshlet_bytes = 30;
    uint8_t *rows = (uint8_t *)std::malloc(rows_bytes), *meshlet = (uint8_t *)std::malloc(meshlet_bytes);
    std::memset(rows, 0, rows_bytes), std::memset(meshlet, 0xEE, meshlet_bytes);
    for (int v = 0; v < 3; v++) {
        const int8_t n[4] = {(int8_t)(127 - 50 * v), (int8_t)(40 * v - 128), 64, 0}, t[4] = {-128, (int8_t)(90 - 60 * v), 17, (int8_t)(v == 1 ? -127 : 127)};
        const float uv[2] = {0.25f * (float)v, 100.0f - 3.0f * (float)v};
        std::memcpy(rows + 32 * v, &pos[3 * v], 12), std::memcpy(rows + 32 * v + 12, n, 4);
        std::memcpy(rows + 32 * v + 16, uv, 8), std::memcpy(rows + 32 * v + 24, t, 4);
    }
    const uint16_t material = 4321;
    std::memcpy(meshlet + 28, &material, 2);
    for (int tampered = 0; tampered < 2; tampered++) {
        std::vector<uint64_t> buf = vis;
        std::vector<float> bary(2 * W * H), grad(4 * W * H);
        std::vector<uint32_t> tri(4 * W * H);
        OrbitVisibilitySurface s{};
        s.visibility = buf.data(), s.draw_commands = cmds.data(), s.meshlet_data = data.data(), s.vertices = pos.data();
        s.entity_data = ent.data(), s.bary = bary.data(), s.grad = grad.data(), s.triangle = tri.data();
        s.meshlet_data_words = data.size(), s.vertex_count = 3, s.max_commands = 1, s.entity_count = 1, s.vertex_stride = 12;
        s.width = W, s.height = H, s.flags = ORBIT_SURFACE_CLEAR;
        std::memcpy(s.view_proj, vp, 64);
        int32_t status = 7;
        raster::visibility_surface_drawn(s, ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD, &status);
        if (status != ORBIT_OK) return 1;
        if (tampered) {
            tri[4 * (4 * W + 30) + 2] = 3;            // g1 = vertex_count
            tri[4 * (4 * W + 31) + 0] = 1;            // entity = entity_count
            tri[4 * (4 * W + 32) + 0] = 0xFFFFFFFFu;  // left out by the surface call
            buf[0] = (0x3f000000ull << 32) | (5u << 8); // a foreign id
        }
        std::vector<float> world_pos(4 * W * H), normal(3 * W * H), tangent(4 * W * H), uv(2 * W * H), uv_grad(4 * W * H);
        std::vector<uint32_t> mat(W * H);
        OrbitFragmentStats st;
        OrbitSurfaceFragments f{};
        f.visibility = buf.data(), f.draw_commands = cmds.data(), f.meshlets = (const OrbitMeshlet *)meshlet;
        f.bary = bary.data(), f.grad = grad.data(), f.triangle = tri.data(), f.vertices = rows, f.entity_data = ent.data();
        f.world_pos = world_pos.data(), f.normal = normal.data(), f.tangent = tangent.data(), f.uv = uv.data(), f.uv_grad = uv_grad.data();
        f.material = mat.data(), f.stats = &st;
        f.vertex_count = 3, f.meshlet_count = 1, f.max_commands = 1, f.entity_count = 1;
        f.vertex_stride = 32, f.position_offset = 0, f.normal_offset = 12, f.uv_offset = 16, f.tangent_offset = 24;
        f.width = W, f.height = H, f.flags = ORBIT_FRAGMENTS_CLEAR;
        raster::surface_fragments(f, &status);
        std::printf("fragments %u, tampered %d: covered %u written %u foreign %u unshaded %u stale %u degenerate %u status %d material %u\n",
                    rs.fragments, tampered, st.covered_pixels, st.written_pixels, st.foreign_pixels, st.unshaded_pixels, st.stale_pixels,
                    st.degenerate_pixels, status, mat[4 * W + 40]);
        if (st.covered_pixels != st.written_pixels + st.foreign_pixels + st.stale_pixels + st.unshaded_pixels) return 1;
        if (mat[4 * W + 40] != material) return 1;
        if (!tampered && (st.written_pixels != st.covered_pixels || st.covered_pixels == 0 || status != ORBIT_OK)) return 1;
        if (tampered && (st.stale_pixels != 2 || st.unshaded_pixels != 1 || st.foreign_pixels != 1 || status != ORBIT_E_RANGE)) return 1;
    }
    std::free(rows), std::free(meshlet);
    return 0;
}
