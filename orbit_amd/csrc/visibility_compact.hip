// visibility_compact.hip — orbit_visibility_compact (include/orbit_abi_ext.h C1-C6): from a visibility
// buffer and the list that produced it to the exact visible draw list, optionally cut down to the visible triangles.
//
// Five launches on the stream, no look-back and no spinning anywhere:
//   clear   triangle_masks, stats, the workspace and the output's count = 0
//   mark    C1.  A wave takes an 8 x 8 pixel tile and aggregates before it touches memory: the first remaining lane's low
//           32 bits (command and triangle), a ballot of the lanes that hold the same, ONE non-returning atomicOr from one
//           lane, behind a relaxed load that skips it where the bit is already set — the masks only grow, so a stale 0
//           costs an atomic, never a bit.  The two counters are wave-uniform popcounts, one atomic each per wave at the end.
//   scan    C2.  A lane per command: the popcount of its eight words, the consistency test, the pair (visible, size);
//           a block's totals go into the workspace.
//   totals  one block turns the blocks' totals into their exclusive carries, in order, and writes the two sums.
//   emit    C3-C5.  A lane per command takes its j and base from block_exclusive_scan plus the block's carry; for each
//           written command of the wave's ballot the whole wave writes it: the seven words, the id, and with
//           ORBIT_COMPACT_TRIANGLES the region, staged in LDS (index words, then the corner bytes of round t = base +
//           lane at 3 * rank, rank from lane_prefix plus the earlier rounds' count) and stored as whole coalesced words:
//           the pad bytes are 0 by construction and there is no byte-granular global store.  What the owning lane read
//           for its verdict (command words, masks) is broadcast, not read again.
#include "kernels.h"
#include "orbit_device.h"
#include "scan.h"

namespace orbit {
namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kChunk = kCompactChunk;   // commands per block of scan and emit: one per lane
constexpr uint32_t kRegionWords = 255 + 192; // vcount <= 255 index words and 256 triangles' corner bytes
static_assert(kChunk == kThreads, "a lane per command");

// OrbitVisibilityCompactStats' order
enum : uint32_t { kCovered, kForeign, kVisible, kTriangles, kWritten, kDropped, kDataWords, kRangeErrors, kStatWords };

// a block's slot of the workspace: before `totals` the block's sums, after it the sums of the blocks in front of it
struct Carry {
    uint32_t visible, _pad;
    unsigned long long words;
};
static_assert(sizeof(Carry) == kCompactCarryBytes, "the workspace's slot");

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void compact_clear_kernel(uint32_t *masks, uint32_t mask_words, uint32_t *workspace,
                                                                 uint32_t workspace_words, uint32_t *stats, uint32_t *out_count) {
    const uint32_t stride = gridDim.x * kThreads, first = blockIdx.x * kThreads + threadIdx.x;
    for (uint32_t i = first; i < mask_words; i += stride) masks[i] = 0u;
    for (uint32_t i = first; i < workspace_words; i += stride) workspace[i] = 0u;
    if (stats && first < kStatWords) stats[first] = 0u;
    if (first == 0u) out_count[0] = 0u;
}

__global__ __launch_bounds__(kThreads) void compact_mark_kernel(const OrbitVisibilityCompact j, const uint32_t tiles_x,
                                                                const uint32_t tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    const uint32_t listed = ((const uint32_t *)j.draw_commands)[0];
    const uint32_t n = listed < j.max_commands ? listed : j.max_commands;
    uint32_t n_covered = 0, n_foreign = 0; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
        const bool in_target = x < j.width && y < j.height;
        const uint64_t word = in_target ? j.visibility[(size_t)y * j.width + x] : 0ull;
        const bool covered = word != 0ull;
        const uint32_t key = (uint32_t)word; // command << 8 | triangle
        const uint32_t k = (key >> 8) - j.command_base; // (below the base it wraps far above n)
        const bool own = covered && k < n;
        n_covered += (uint32_t)__popcll(__ballot(covered));
        n_foreign += (uint32_t)__popcll(__ballot(covered && !own));
        uint64_t left = __ballot(own);
        while (left != 0ull) {
            const uint32_t src = (uint32_t)__builtin_ctzll(left);
            const uint32_t key_src = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)src);
            left &= ~__ballot(own && key == key_src);
            if (lane == src) { // k < n <= max_commands: inside the 8 * max_commands words
                uint32_t *dst = j.triangle_masks + 8u * (size_t)k + ((key & 255u) >> 5);
                const uint32_t bit = 1u << (key & 31u);
                if (!(__hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
                    (void)__hip_atomic_fetch_or(dst, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (!j.stats || lane != 0u) return;
    uint32_t *stats = (uint32_t *)j.stats;
    if (n_covered != 0u) atomicAdd(&stats[kCovered], n_covered);
    if (n_foreign != 0u) atomicAdd(&stats[kForeign], n_foreign);
}

// C2 of command k < n: what the scan and the emit both need of it, computed alike
struct Verdict {
    bool visible;    // its mask is non-zero
    bool consistent; // (meaningful when visible)
    uint32_t m, vcount, size;
    uint32_t first_index, index_base, mask[8]; // kept for the emit: it reads none of them a second time
};
constexpr Verdict kNoVerdict{false, false, 0u, 0u, 0u, 0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};

__device__ __forceinline__ Verdict verdict_of(const OrbitVisibilityCompact &j, uint32_t k) {
    const uint32_t *mask = j.triangle_masks + 8u * (size_t)k;
    const uint32_t *cmd = (const uint32_t *)j.draw_commands + 1u + 7u * (size_t)k;
    Verdict v = kNoVerdict;
    const uint32_t index_count = cmd[0], first_index = cmd[2], index_base = cmd[3];
    v.first_index = first_index, v.index_base = index_base;
    const uint32_t nt = index_count / 3u, first_word = first_index / 4u;
    uint32_t beyond = 0; // mask bits t >= nt
#pragma unroll
    for (uint32_t w = 0; w < 8u; w++) {
        const uint32_t bits = v.mask[w] = mask[w];
        v.m += (uint32_t)__popc(bits);
        const uint32_t valid = nt > 32u * w ? nt - 32u * w : 0u; // triangles of this word
        beyond |= valid >= 32u ? 0u : bits & ~((1u << valid) - 1u);
    }
    v.visible = v.m != 0u;
    v.consistent = nt <= 256u && beyond == 0u;
    if (j.flags & ORBIT_COMPACT_TRIANGLES) {
        v.vcount = first_word - index_base; // (meaningful once first_word >= index_base)
        // R9's checks that concern meshlet_data, the expressions of raster_walk.h
        const bool bad = first_word < index_base || v.vcount > 255u || (uint64_t)first_word > j.meshlet_data_words ||
                         ((uint64_t)first_index + 3ull * nt + 3ull) / 4ull > j.meshlet_data_words;
        v.consistent = v.consistent && !bad;
        v.size = v.vcount + (3u * v.m + 3u) / 4u;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void compact_scan_kernel(const OrbitVisibilityCompact j, int32_t *status) {
    __shared__ uint32_t smem[kWaves + 1];
    const uint32_t listed = ((const uint32_t *)j.draw_commands)[0];
    const uint32_t n = listed < j.max_commands ? listed : j.max_commands;
    const uint32_t k = blockIdx.x * kChunk + threadIdx.x;
    Verdict v = kNoVerdict;
    if (k < n) v = verdict_of(j, k);
    const bool keep = v.visible && v.consistent, error = v.visible && !v.consistent;
    uint32_t visible, words, triangles, errors; // a block holds at most 256 * 447 words: 32 bits do
    (void)block_exclusive_scan<kWaves>(keep ? 1u : 0u, smem, &visible);
    (void)block_exclusive_scan<kWaves>(keep ? v.size : 0u, smem, &words);
    (void)block_exclusive_scan<kWaves>(keep ? v.m : 0u, smem, &triangles);
    (void)block_exclusive_scan<kWaves>(error ? 1u : 0u, smem, &errors);
    if (threadIdx.x != 0u) return;
    Carry *carry = (Carry *)j.workspace + blockIdx.x;
    carry->visible = visible, carry->words = words;
    if (errors != 0u) latch_status(status, ORBIT_E_RANGE);
    if (!j.stats) return;
    uint32_t *stats = (uint32_t *)j.stats;
    if (triangles != 0u) atomicAdd(&stats[kTriangles], triangles);
    if (errors != 0u) atomicAdd(&stats[kRangeErrors], errors);
}

// one block: the blocks' totals -> the totals of the blocks in front of each, and the two sums
__global__ __launch_bounds__(kThreads) void compact_totals_kernel(const OrbitVisibilityCompact j, const uint32_t blocks) {
    __shared__ uint32_t smem[kWaves + 1];
    Carry *carry = (Carry *)j.workspace;
    uint32_t visible_before = 0;
    unsigned long long words_before = 0; // 2^24 commands of 447 words do not fit 32 bits
    for (uint32_t first = 0; first < blocks; first += kThreads) { // (block-uniform)
        const uint32_t b = first + threadIdx.x;
        const uint32_t visible = b < blocks ? carry[b].visible : 0u;
        const uint32_t words = b < blocks ? (uint32_t)carry[b].words : 0u; // (a block's own total: below 2^17)
        uint32_t visible_sum, words_sum; // 256 blocks' totals: below 2^25
        const uint32_t visible_ex = block_exclusive_scan<kWaves>(visible, smem, &visible_sum);
        const uint32_t words_ex = block_exclusive_scan<kWaves>(words, smem, &words_sum);
        if (b < blocks) carry[b].visible = visible_before + visible_ex, carry[b].words = words_before + words_ex;
        visible_before += visible_sum, words_before += words_sum;
    }
    if (threadIdx.x != 0u) return;
    carry[blocks].visible = visible_before, carry[blocks].words = words_before; // the sums, for the emit's blocks
    if (!j.stats) return;
    uint32_t *stats = (uint32_t *)j.stats;
    stats[kVisible] = visible_before;
    stats[kDataWords] = words_before > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)words_before;
}

__global__ __launch_bounds__(kThreads) void compact_emit_kernel(const OrbitVisibilityCompact j, int32_t *status) {
    __shared__ uint32_t smem[kWaves + 1];
    __shared__ uint32_t lds_region[kWaves][kRegionWords + 1];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool cut = (j.flags & ORBIT_COMPACT_TRIANGLES) != 0u;
    const uint32_t *commands = (const uint32_t *)j.draw_commands;
    uint32_t *out = (uint32_t *)j.visible_commands;
    const uint32_t listed = commands[0];
    const uint32_t n = listed < j.max_commands ? listed : j.max_commands;
    if (blockIdx.x * kChunk >= n) return; // (block-uniform) nothing listed here: nothing visible
    const uint32_t k = blockIdx.x * kChunk + threadIdx.x;
    Verdict v = kNoVerdict;
    if (k < n) v = verdict_of(j, k);
    const bool keep = v.visible && v.consistent;
    const Carry carry = ((const Carry *)j.workspace)[blockIdx.x];
    uint32_t unused;
    const uint32_t jv = carry.visible + block_exclusive_scan<kWaves>(keep ? 1u : 0u, smem, &unused);
    const unsigned long long base64 = carry.words + block_exclusive_scan<kWaves>(keep ? v.size : 0u, smem, &unused);
    // C3.  (base64 + size <= visible_data_words <= 2^30: a written command's base fits 32 bits)
    const bool written = keep && jv < j.visible_capacity && (!cut || base64 + v.size <= (unsigned long long)j.visible_data_words);
    const uint32_t base = (uint32_t)base64;
    const uint64_t written_lanes = __ballot(written), dropped_lanes = __ballot(keep && !written);
    if (lane == 0u) {
        if (written_lanes != 0ull) atomicAdd(&out[0], (uint32_t)__popcll(written_lanes));
        if (dropped_lanes != 0ull) latch_status(status, ORBIT_E_CAPACITY);
        if (j.stats) {
            uint32_t *stats = (uint32_t *)j.stats;
            if (written_lanes != 0ull) atomicAdd(&stats[kWritten], (uint32_t)__popcll(written_lanes));
            if (dropped_lanes != 0ull) atomicAdd(&stats[kDropped], (uint32_t)__popcll(dropped_lanes));
        }
    }
    uint32_t *region = lds_region[wave];
    uint8_t *region_bytes = (uint8_t *)region;
    const uint8_t *data_bytes = (const uint8_t *)j.meshlet_data;
    uint64_t left = written_lanes;
    while (left != 0ull) { // (wave-uniform) the whole wave writes one command
        const uint32_t src = (uint32_t)__builtin_ctzll(left);
        left &= left - 1ull;
        const uint32_t k_src = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)src);
        const uint32_t j_src = (uint32_t)__builtin_amdgcn_readlane((int)jv, (int)src);
        const uint32_t *cmd = commands + 1u + 7u * (size_t)k_src;
        if (!cut) { // C4.  (j_src < visible_capacity: inside the output)
            if (lane < 7u) out[1u + 7u * (size_t)j_src + lane] = cmd[lane];
            if (lane == 7u && j.visible_ids) j.visible_ids[j_src] = j.command_base + k_src;
            continue;
        }
        // C5
        const uint32_t base_src = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)src);
        const uint32_t m_src = (uint32_t)__builtin_amdgcn_readlane((int)v.m, (int)src);
        const uint32_t vcount = (uint32_t)__builtin_amdgcn_readlane((int)v.vcount, (int)src);
        const uint32_t corner_words = (3u * m_src + 3u) / 4u, size = vcount + corner_words; // size <= kRegionWords
        if (lane < 7u) {
            uint32_t word = cmd[lane];
            if (lane == 0u) word = 3u * m_src;
            if (lane == 2u) word = 4u * (base_src + vcount);
            if (lane == 3u) word = base_src;
            out[1u + 7u * (size_t)j_src + lane] = word;
        }
        if (lane == 7u && j.visible_ids) j.visible_ids[j_src] = j.command_base + k_src;
        // (the verdict checked both ranges of meshlet_data, and that no set bit lies at or beyond nt.)  What the owning
        // lane read for its verdict is broadcast, and every load of the region is issued before the first is used: a
        // command costs one trip to memory, not one per step
        const uint32_t index_base = (uint32_t)__builtin_amdgcn_readlane((int)v.index_base, (int)src);
        const uint32_t first_index = (uint32_t)__builtin_amdgcn_readlane((int)v.first_index, (int)src);
        uint32_t index_words[4], corners[4], ranks[4], earlier = 0; // earlier: set bits of the rounds before this one
        uint64_t bits[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) { // vcount <= 255: four words per lane at most
            const uint32_t i = 64u * q + lane;
            index_words[q] = i < vcount ? j.meshlet_data[(size_t)index_base + i] : 0u;
        }
#pragma unroll
        for (uint32_t round = 0; round < 4u; round++) { // triangle t = 64 * round + lane
            bits[round] = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v.mask[2u * round], (int)src) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v.mask[2u * round + 1u], (int)src) << 32;
            ranks[round] = earlier + lane_prefix(bits[round]);
            earlier += (uint32_t)__popcll(bits[round]);
            corners[round] = 0u;
            if ((bits[round] >> lane) & 1ull) {
                const uint8_t *c = data_bytes + (size_t)first_index + 3u * (size_t)(64u * round + lane);
                corners[round] = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++)
            if (64u * q + lane < vcount) region[64u * q + lane] = index_words[q];
        for (uint32_t i = lane; i < corner_words; i += 64u) region[vcount + i] = 0u;
        wave_lds_sync();
#pragma unroll
        for (uint32_t round = 0; round < 4u; round++)
            if ((bits[round] >> lane) & 1ull) {
                uint8_t *dst = region_bytes + 4u * (size_t)vcount + 3u * (size_t)ranks[round]; // rank < m_src: inside the corner words
                dst[0] = (uint8_t)corners[round], dst[1] = (uint8_t)(corners[round] >> 8), dst[2] = (uint8_t)(corners[round] >> 16);
            }
        wave_lds_sync();
        // (base_src + size <= visible_data_words: inside the output)
        for (uint32_t i = lane; i < size; i += 64u) j.visible_data[(size_t)base_src + i] = region[i];
        wave_lds_sync(); // the next command overwrites the wave's LDS
    }
}

} // namespace

hipError_t launch_visibility_compact(const OrbitVisibilityCompact &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status,
                                     hipStream_t s) {
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const uint32_t blocks = (job.max_commands + kChunk - 1u) / kChunk; // max_commands <= 2^24: at most 65536
    {
        // 8 * max_commands <= 2^27 mask words
        const uint32_t mask_words = 8u * job.max_commands, workspace_words = (blocks + 1u) * (kCompactCarryBytes / 4u);
        const uint32_t most = mask_words > workspace_words ? mask_words : workspace_words;
        const uint32_t need = (most + kThreads * 4u - 1u) / (kThreads * 4u);
        hipLaunchKernelGGL(compact_clear_kernel, dim3(need < 1u ? 1u : need < cap ? need : cap), dim3(kThreads), 0, s,
                           job.triangle_masks, mask_words, (uint32_t *)job.workspace, workspace_words, (uint32_t *)job.stats,
                           (uint32_t *)job.visible_commands);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    {
        // width, height <= 32768: at most 2^24 tiles
        const uint32_t tiles_x = (job.width + 7u) / 8u, tiles = tiles_x * ((job.height + 7u) / 8u);
        const uint32_t need = (tiles + kWaves - 1u) / kWaves;
        hipLaunchKernelGGL(compact_mark_kernel, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (blocks == 0u) return hipSuccess; // no command: the list stays empty
    hipLaunchKernelGGL(compact_scan_kernel, dim3(blocks), dim3(kThreads), 0, s, job, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compact_totals_kernel, dim3(1), dim3(kThreads), 0, s, job, blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compact_emit_kernel, dim3(blocks), dim3(kThreads), 0, s, job, status);
    return hipGetLastError();
}

} // namespace orbit
